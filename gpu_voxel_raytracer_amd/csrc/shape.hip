// shape.hip — device side of vxrt_shape.h: the tiles that meet the box, keyed (shape_tiles_kernel), and one block per tile in path
// order that counts, then writes, the tile's cells inside the shape (shape_kernel).  The host side is api_shape.hip; the rule's
// arithmetic is shape_rule.h's, the kernels' contract is in shape.h and the argument in DESIGN.md §29.
//
// Path order without a sort over the result: a path key's low 12 bits walk one aligned 16^3 tile, so with the tiles in ascending
// key order (the caller sorts their 36-bit keys) and thread t of a block holding the tile's path indices 16 t .. 16 t + 15, the
// block's exclusive scan in thread order numbers the tile's voxels in path order, and the scan over the tiles' counts places the
// tiles.  Every byte written is a function of the shape, the map, the box and the cell alone; the counts are integer sums in thread
// order.  Bounds: every loop runs a fixed count (kShapeItems cells, 8 corners, 3 axes); no workgroup waits for another; no atomics.
//
// Two shortcuts decide for a tile as one — they depend on blockIdx and the arguments alone — and neither changes a byte:
//   wholly outside  per shape axis the pulled P_i of rule 1 over the cells of (tile ∩ box) lies between the sums of its terms' least
//                   and greatest values, each term being monotonic in its coordinate (block_misses_source's argument,
//                   transform.hip), and those two sums are P_i at two of the 8 corner cells.  Where that interval misses
//                   [-reach_i, reach_i], the shape's extent on the axis (R, H_i, or H_2 + R along a capsule), every cell fails
//                   rule 3 on that axis alone: P_i^2 > R^2, or P_i outside [-H_i, H_i).
//   wholly inside   the set of real P that pass rules 2 and 3 is convex (an open cube cut with a half-open box, a ball, a cylinder
//                   or a capsule — the points within R of a segment), the integer tests decide membership of it exactly (no sum
//                   wraps), and P is an affine function of the cell.  Every cell of (tile ∩ box), itself a box of cells, is a convex
//                   combination of that box's 8 corner cells, so its P is the same combination of theirs: where the 8 corners
//                   pass, every cell passes, and the count is the product of the clipped extents.
// The counting pass leaves what it found in the top bits of the tile's key; the emitting pass reads it there.
#include "block_scan.h"
#include "shape.h"
#include "shape_rule.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kShapeThreads / 64;

// -DVXRT_SHAPE_NO_OUTSIDE, -DVXRT_SHAPE_NO_INSIDE, -DVXRT_SHAPE_NO_SHORTCUTS (both) — A/B builds, scripts/ab_build.sh: tiles evaluate
// their cells where a shortcut would have decided — what each shortcut is measured against
#if defined(VXRT_SHAPE_NO_SHORTCUTS) || defined(VXRT_SHAPE_NO_OUTSIDE)
constexpr bool kOutsideTest = false;
#else
constexpr bool kOutsideTest = true;
#endif
#if defined(VXRT_SHAPE_NO_SHORTCUTS) || defined(VXRT_SHAPE_NO_INSIDE)
constexpr bool kInsideTest = false;
#else
constexpr bool kInsideTest = true;
#endif

__global__ __launch_bounds__(kShapeThreads) void shape_tiles_kernel(const ShapeArgs a) {
    const uint32_t i = blockIdx.x * kShapeThreads + threadIdx.x;
    if (i >= a.tiles) return;
    const uint32_t yz = a.text[1] * a.text[2];      // at most 4097^2
    const uint32_t x = i / yz, r = i - x * yz, y = r / a.text[2], z = r - y * a.text[2];
    a.keys[i] = spread16(a.tlo[0] + x) << 2 | spread16(a.tlo[1] + y) << 1 | spread16(a.tlo[2] + z);
}

// lo .. hi (inclusive): the cells of (tile ∩ box).  Nobody evaluates 8 corners: lane l of every wave pulls corner l & 7, and wave
// votes join them.  P_i is affine in the cell, so its least and greatest values over the box of cells are taken at corners: "every
// corner's P_i is below -reach_i" is the interval test's "most < -reach_i", and likewise above.  Every wave of the block votes on
// the same 8 corners, so all reach the same verdict without a barrier.
__device__ __forceinline__ uint64_t tile_class(const ShapeArgs& a, const int32_t* lo, const int32_t* hi) {
    if (!kOutsideTest && !kInsideTest) return kShapeMixed;
    const uint32_t k = threadIdx.x & 7u;
    const int32_t d[3] = {(k & 4u) ? hi[0] : lo[0], (k & 2u) ? hi[1] : lo[1], (k & 1u) ? hi[2] : lo[2]};
    int64_t p[3];
    shape_pull(a.m, a.t, d, p);
    if (kOutsideTest) {
        bool miss = false;
#pragma unroll
        for (int i = 0; i < 3; i++) miss = miss || __all(p[i] < -a.reach[i] ? 1 : 0) || __all(p[i] > a.reach[i] ? 1 : 0);
        if (miss) return kShapeOutside;
    }
    if (kInsideTest && __all(shape_inside(a.kind, a.r2, a.h2, p) ? 1 : 0)) return kShapeWhole;
    return kShapeMixed;
}

__device__ __forceinline__ void store_voxel(const ShapeArgs& a, uint64_t at, const int32_t* d) {
    uint8_t* o = a.out_pos + 6 * size_t(at);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        o[2 * ax] = uint8_t(uint32_t(d[ax]) & 0xffu);
        o[2 * ax + 1] = uint8_t((uint32_t(d[ax]) >> 8) & 0xffu);
    }
    if (a.out_mrgb != nullptr) {
        uint8_t* b = a.out_mrgb + 4 * size_t(at);
        b[0] = uint8_t((a.word >> 24) & 0x7fu);
        b[1] = uint8_t((a.word >> 16) & 0xffu);
        b[2] = uint8_t((a.word >> 8) & 0xffu);
        b[3] = uint8_t(a.word & 0xffu);
    }
}

// Path index 16 t + j of a tile is the cell whose x, y and z have the index's bits 3k + 2, 3k + 1 and 3k: thread t holds the
// 2 x 2 x 4 brick at (compact16(16 t >> 2), compact16(16 t >> 1), compact16(16 t)), and j's bits 2, 1, 0 and 3 are the brick's x0,
// y0, z0 and z1.  The 16 cells are evaluated one after another into a bit mask: three 64-bit sums live at a time, not 48.
template <bool kEmit>
__global__ __launch_bounds__(kShapeThreads) void shape_kernel(const ShapeArgs a) {
    const uint64_t entry = a.keys[blockIdx.x];
    const uint64_t key = entry & kShapeTileMask;
    int32_t lo[3], hi[3], org[3];
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        org[ax] = int32_t(compact16(key >> (2 - ax)) << 4) - 32768;
        lo[ax] = max(org[ax], a.lo[ax]);
        hi[ax] = min(org[ax] + 15, a.hi[ax] - 1);      // lo <= hi: the tile meets the box
    }
    uint64_t cls;
    if (kEmit) {
        cls = entry >> kShapeClassShift;
        if (cls == kShapeOutside) return;
    } else {
        cls = tile_class(a, lo, hi);
        if (cls != kShapeMixed) {
            if (threadIdx.x == 0) {
                a.part[blockIdx.x] = cls == kShapeWhole ? uint64_t(hi[0] - lo[0] + 1) * uint64_t(hi[1] - lo[1] + 1) * uint64_t(hi[2] - lo[2] + 1) : 0u;
                a.keys[blockIdx.x] = key | cls << kShapeClassShift;
            }
            return;
        }
    }

    const uint32_t first = threadIdx.x * kShapeItems;
    const int32_t b[3] = {org[0] + int32_t(compact16(first >> 2)), org[1] + int32_t(compact16(first >> 1)), org[2] + int32_t(compact16(first))};
    int64_t pb[3];
    shape_pull(a.m, a.t, b, pb);
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t j = 0; j < kShapeItems; j++) {
        const int32_t e[3] = {int32_t((j >> 2) & 1u), int32_t((j >> 1) & 1u), int32_t((j & 1u) | ((j >> 3) & 1u) << 1)};
        bool in = true;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) in = in && b[ax] + e[ax] >= lo[ax] && b[ax] + e[ax] <= hi[ax];
        if (cls != kShapeWhole) {
            int64_t p[3];
#pragma unroll
            for (int i = 0; i < 3; i++) p[i] = pb[i] + 2 * (int64_t(a.m[i][0]) * e[0] + int64_t(a.m[i][1]) * e[1] + int64_t(a.m[i][2]) * e[2]);
            in = in && shape_inside(a.kind, a.r2, a.h2, p);
        }
        mask |= in ? 1u << j : 0u;
    }
    const uint32_t mine = uint32_t(__popc(mask));
    if (!kEmit) {
        block_sum_to<kWaves>(mine, a.part + blockIdx.x);
        return;
    }
    __shared__ uint32_t scan[kWaves];
    uint32_t total;
    uint64_t to = a.part[blockIdx.x] + block_exclusive<uint32_t, kWaves>(mine, scan, &total);
#pragma unroll
    for (uint32_t j = 0; j < kShapeItems; j++) {
        if (mask >> j & 1u) {
            const int32_t d[3] = {b[0] + int32_t((j >> 2) & 1u), b[1] + int32_t((j >> 1) & 1u), b[2] + int32_t((j & 1u) | ((j >> 3) & 1u) << 1)};
            store_voxel(a, to, d);
            to++;
        }
    }
}

#ifdef VXRT_SHAPE_SORTED
template <bool kEmit>
__global__ __launch_bounds__(kShapeThreads) void shape_linear_kernel(const ShapeArgs a) {
    const uint32_t c0 = blockIdx.x * kShapeSpan;
    const uint32_t yz = a.ext[1] * a.ext[2];
    uint32_t mask = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        const uint32_t c = c0 + j * kShapeThreads + threadIdx.x;
        const uint32_t cc = c < a.cells ? c : a.cells - 1u;
        const uint32_t x = cc / yz, r = cc - x * yz, y = r / a.ext[2], z = r - y * a.ext[2];
        const int32_t d[3] = {a.lo[0] + int32_t(x), a.lo[1] + int32_t(y), a.lo[2] + int32_t(z)};
        int64_t p[3];
        shape_pull(a.m, a.t, d, p);
        mask |= c < a.cells && shape_inside(a.kind, a.r2, a.h2, p) ? 1u << j : 0u;
    }
    const uint32_t mine = uint32_t(__popc(mask));
    if (!kEmit) {
        block_sum_to<kWaves>(mine, a.part + blockIdx.x);
        return;
    }
    __shared__ uint32_t scan[kWaves];
    uint32_t total;
    uint64_t to = a.part[blockIdx.x] + block_exclusive<uint32_t, kWaves>(mine, scan, &total);
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) {
        if (mask >> j & 1u) {
            const uint32_t c = c0 + j * kShapeThreads + threadIdx.x;
            const uint32_t x = c / yz, r = c - x * yz, y = r / a.ext[2], z = r - y * a.ext[2];
            a.out_keys[to++] = path_key15(a.lo[0] + int32_t(x), a.lo[1] + int32_t(y), a.lo[2] + int32_t(z));
        }
    }
}

__global__ __launch_bounds__(kShapeThreads) void shape_decode_kernel(const uint64_t* keys, uint32_t n, ShapeArgs a) {
    const uint32_t i = blockIdx.x * kShapeThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    const int32_t d[3] = {int32_t(compact16(k >> 2)) - 32768, int32_t(compact16(k >> 1)) - 32768, int32_t(compact16(k)) - 32768};
    store_voxel(a, i, d);
}
#endif

}  // namespace

hipError_t launch_shape_tiles(const ShapeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(shape_tiles_kernel, dim3((a.tiles + kShapeThreads - 1) / kShapeThreads), dim3(kShapeThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shape(const ShapeArgs& a, hipStream_t s) {
    const dim3 grid(a.tiles), block(kShapeThreads);
    if (a.out_pos != nullptr)
        hipLaunchKernelGGL(shape_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(shape_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

#ifdef VXRT_SHAPE_SORTED
hipError_t launch_shape_linear(const ShapeArgs& a, hipStream_t s) {
    const dim3 grid(shape_blocks(a.cells)), block(kShapeThreads);
    if (a.out_keys != nullptr)
        hipLaunchKernelGGL(shape_linear_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(shape_linear_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_shape_decode(const uint64_t* keys, uint32_t n, uint32_t word, uint8_t* pos, uint8_t* mrgb, hipStream_t s) {
    ShapeArgs a{};
    a.out_pos = pos;
    a.out_mrgb = mrgb;
    a.word = word;
    hipLaunchKernelGGL(shape_decode_kernel, dim3((n + kShapeThreads - 1) / kShapeThreads), dim3(kShapeThreads), 0, s, keys, n, a);
    return hipGetLastError();
}
#endif

}  // namespace vxrt
