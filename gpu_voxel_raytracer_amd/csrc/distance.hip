// distance.hip — device side of vxrt_distance.h: the run heads of a sorted key array, which give the tiles of a list and, spread over
// their 3 x 3 x 3 windows and sorted, the candidate tiles (distance_heads_kernel), and one block per candidate tile in path order that
// evaluates the exact squared Euclidean distance of the tile's 4096 cells in three separable passes over an occupancy image in LDS and
// counts, then writes, the cells the mode asks for (distance_kernel).  The host side is api_distance.hip; the rule's arithmetic is
// distance_rule.h's, the kernels' contract is in distance.h and the argument in DESIGN.md §30.
//
// Unique result: the occupancy image is built with OR, which commutes; every value after it is a function of the image, the mode and
// max_d2 alone, and the passes visit their offsets in rank order and keep a strictly smaller value, so ties fall as rule 5 says; the
// counts are integer sums in thread order.  Path order without a sort over the result: shape.hip's scheme — the tiles ascend, thread t
// holds the tile's path indices 16 t .. 16 t + 15, and the block's exclusive scan numbers the cells.  Bounds: every loop runs a fixed
// count or one bounded by the radius (at most 16) or a run's length (at most 4096 voxels a tile); no workgroup waits for another; no
// global atomics.  Every global load is issued by every lane from an index clamped into its array, whether or not its value is used.
#include "block_scan.h"
#include "distance.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kDistanceThreads / 64;
constexpr uint32_t kCentre = 13;      // the window's own tile: (0, 0, 0)

template <bool kEmit>
__global__ __launch_bounds__(kDistanceThreads) void distance_heads_kernel(const uint64_t* keys, uint32_t n, uint32_t shift, bool spread,
                                                                          uint64_t* part, uint64_t* out) {
    const uint64_t i = uint64_t(blockIdx.x) * kDistanceThreads + threadIdx.x;
    const uint32_t at = i < n ? uint32_t(i) : n - 1u, before = at != 0u ? at - 1u : 0u;      // n > 0
    const uint64_t key = keys[at] >> shift, prev = keys[before] >> shift;
    const uint32_t head = i < n && (i == 0u || key != prev) ? 1u : 0u;
    if (!kEmit) {
        block_sum_to<kWaves>(head, part + blockIdx.x);
        return;
    }
    __shared__ uint32_t scan[kWaves];
    uint32_t total;
    const uint64_t to = part[blockIdx.x] + block_exclusive<uint32_t, kWaves>(head, scan, &total);
    if (head == 0u) return;
    if (!spread) {
        out[to] = key;
        return;
    }
    for (uint32_t w = 0; w < kDistanceWindowTiles; w++) {
        bool ok;
        out[to * kDistanceWindowTiles + w] = distance_window_tile(key, w, &ok);
    }
}

__device__ __forceinline__ void store16(uint8_t* o, uint32_t v) {
    o[0] = uint8_t(v & 0xffu);
    o[1] = uint8_t((v >> 8) & 0xffu);
}

// kInvert: DEPTH and ERODE, which measure to the nearest empty cell: the image's rows are complemented as they are read, and a cell
// outside the int16 range, where nothing was scattered, reads as empty (rule 3).
template <bool kInvert, bool kEmit>
__global__ __launch_bounds__(kDistanceThreads) void distance_kernel(const DistanceArgs a) {
    __shared__ uint64_t rows[kDistanceRows];                  // the occupancy image: row (wz, wy) at wz W + wy, bit wx
    __shared__ uint16_t slab[kDistanceSlab];                  // pass 2: d2 within the plane, at (wz 16 + y) 16 + x
    __shared__ int8_t slab_dy[kDistanceSlab];                 // ... and the dy it chose
    __shared__ int8_t plane[kWaves][kDistancePlane];          // pass 1: dx, at wy 16 + x, one plane per wave
    __shared__ uint32_t run_lo[kDistanceWindowTiles], run_hi[kDistanceWindowTiles];
    __shared__ uint64_t run_tile[kDistanceWindowTiles];

    const uint32_t t = threadIdx.x, wave = t >> 6, lane = t & 63u;
    const uint32_t R = a.radius, W = kDistanceTile + 2u * R;
    const uint64_t tile = a.tiles[blockIdx.x];
    const uint32_t last = a.m - 1u;

    // the runs of the window's 27 tiles in the list: two lower bounds each, walked by every thread, kept by the first 54
    {
        const uint32_t w = t < 2u * kDistanceWindowTiles ? t >> 1 : kDistanceWindowTiles - 1u;
        bool ok;
        const uint64_t nt = distance_window_tile(tile, w, &ok);
        const uint32_t found = distance_lower_bound(a.keys, a.m, a.steps, (nt + (t & 1u)) << 12);
        if (t < 2u * kDistanceWindowTiles) {
            if (t & 1u) {
                run_hi[w] = ok ? found : 0u;
            } else {
                run_lo[w] = ok ? found : 0u;
                run_tile[w] = nt;
            }
        }
    }
    for (uint32_t e = t; e < W * W; e += kDistanceThreads) rows[e] = 0u;
    __syncthreads();

    // the image: every voxel of the 27 runs that lies in the window sets its bit
    for (uint32_t w = 0; w < kDistanceWindowTiles; w++) {
        const uint32_t lo = run_lo[w], hi = run_hi[w];
        const int ox = (int(w / 9u) - 1) * 16 + int(R), oy = (int(w / 3u % 3u) - 1) * 16 + int(R), oz = (int(w % 3u) - 1) * 16 + int(R);
        for (uint32_t c = 0; c < kDistanceItems; c++) {
            const uint64_t i = uint64_t(lo) + c * kDistanceThreads + t;
            if (uint64_t(lo) + c * kDistanceThreads >= hi) break;      // the same for the whole block
            const uint64_t key = a.keys[i < last ? uint32_t(i) : last];
            uint32_t x, y, z;
            distance_cell_of(uint32_t(key) & 4095u, &x, &y, &z);
            const uint32_t wx = uint32_t(int(x) + ox), wy = uint32_t(int(y) + oy), wz = uint32_t(int(z) + oz);      // negative: huge
            if (i < hi && wx < W && wy < W && wz < W) atomicOr(reinterpret_cast<unsigned long long*>(&rows[wz * W + wy]), 1ull << wx);
        }
    }
    __syncthreads();

    // passes 1 and 2, plane by plane: wave w takes planes w, w + 4, ...
    const uint64_t row_bits = (uint64_t(1) << W) - 1u;      // W <= 48
    for (uint32_t it = 0; it < (W + kWaves - 1u) / kWaves; it++) {      // at most 12 rounds, the same for the whole block
        const uint32_t wz = it * kWaves + wave;
        if (wz < W) {
#pragma unroll
            for (uint32_t k = 0; k < kDistancePlane / 64u; k++) {
                const uint32_t e = k * 64u + lane, wy = e >> 4, x = e & 15u;
                if (wy < W) {
                    const uint64_t row = (kInvert ? ~rows[wz * W + wy] : rows[wz * W + wy]) & row_bits;
                    plane[wave][e] = int8_t(distance_nearest(row, x + R, R));
                }
            }
        }
        __syncthreads();
        if (wz < W) {
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t y = (lane >> 4) + 4u * k, x = lane & 15u;
                uint32_t best = kDistanceFar;
                int best_dy = 0;
                for (uint32_t rank = 0; rank <= 2u * R; rank++) {
                    const int dy = distance_offset(rank);
                    distance_take_row(int(plane[wave][uint32_t(int(y + R) + dy) * 16u + x]), dy, &best, &best_dy);
                }
                slab[(wz * 16u + y) * 16u + x] = uint16_t(best);
                if (!kInvert) slab_dy[(wz * 16u + y) * 16u + x] = int8_t(best_dy);      // read back for a new cell's source only
            }
        }
        __syncthreads();
    }

    // pass 3: the thread's 16 cells, path indices 16 t .. 16 t + 15
    uint32_t mask = 0, in_set = 0;
    uint32_t found[kDistanceItems];      // d2 | (dz + 16) << 16
#pragma unroll
    for (uint32_t j = 0; j < kDistanceItems; j++) {
        uint32_t x, y, z;
        distance_cell_of(t * kDistanceItems + j, &x, &y, &z);
        uint32_t best = kDistanceFar;
        int best_dz = 0;
        for (uint32_t rank = 0; rank <= 2u * R; rank++) {
            const int dz = distance_offset(rank);
            distance_take_plane(slab[(uint32_t(int(z + R) + dz) * 16u + y) * 16u + x], dz, &best, &best_dz);
        }
        const bool is_set = (rows[(z + R) * W + y + R] >> (x + R) & 1u) != 0u;
        in_set |= is_set ? 1u << j : 0u;
        mask |= distance_emits(a.mode, is_set, best, a.max_d2) ? 1u << j : 0u;
        found[j] = distance_value(best, a.max_d2) | uint32_t(best_dz + 16) << 16;
    }
    const uint32_t mine = uint32_t(__popc(mask));
    if (!kEmit) {
        block_sum_to<kWaves>(mine, a.part + blockIdx.x);
        return;
    }

    __shared__ uint32_t scan[kWaves];
    uint32_t total;
    uint64_t to = a.part[blockIdx.x] + block_exclusive<uint32_t, kWaves>(mine, scan, &total);
    const bool bytes = a.out_mrgb != nullptr;      // uniform
    // DEPTH and ERODE give a voxel its own bytes: the tile's voxels stand in its run in path order, so a voxel's place in the run
    // is the number of voxels before it in the tile
    uint32_t own = 0;
    if (kInvert && bytes) own = run_lo[kCentre] + block_exclusive<uint32_t, kWaves>(uint32_t(__popc(in_set)), scan, &total);
    const int32_t org[3] = {int32_t(distance_compact12(tile >> 2) << 4) - 32768, int32_t(distance_compact12(tile >> 1) << 4) - 32768,
                            int32_t(distance_compact12(tile) << 4) - 32768};
#pragma unroll
    for (uint32_t j = 0; j < kDistanceItems; j++) {
        const bool on = (mask >> j & 1u) != 0u;
        uint32_t x, y, z;
        distance_cell_of(t * kDistanceItems + j, &x, &y, &z);
        uint32_t word = 0;
        if (bytes) {
            uint32_t at;
            if (kInvert) {
                at = own;
                own += in_set >> j & 1u;
            } else {
                // FIELD and DILATE: the source is read back from the passes' choices: dz here, dy in the slab, dx from the row
                const int dz = on ? int(found[j] >> 16) - 16 : 0;
                const uint32_t wz = uint32_t(int(z + R) + dz);
                const int dy = on ? int(slab_dy[(wz * 16u + y) * 16u + x]) : 0;
                const uint32_t wy = uint32_t(int(y + R) + dy);
                const int step = distance_nearest(rows[wz * W + wy] & row_bits, x + R, R);
                const int dx = on ? step : 0;
                const int sx = int(x) + dx, sy = int(y) + dy, sz = int(z) + dz;      // -16 .. 31
                const uint32_t w = on ? uint32_t((sx >> 4) + 1) * 9u + uint32_t((sy >> 4) + 1) * 3u + uint32_t((sz >> 4) + 1) : kCentre;
                const uint64_t q = run_tile[w] << 12 | distance_index_of(uint32_t(sx) & 15u, uint32_t(sy) & 15u, uint32_t(sz) & 15u);
                at = distance_walk(a.keys, last, run_lo[w], on ? run_hi[w] : run_lo[w], 12u, q);
            }
            word = a.words[at < last ? at : last];
        }
        if (on) {
            uint8_t* o = a.out_pos + 6 * size_t(to);
            store16(o, uint32_t(org[0] + int32_t(x)));
            store16(o + 2, uint32_t(org[1] + int32_t(y)));
            store16(o + 4, uint32_t(org[2] + int32_t(z)));
            if (bytes) {
                uint8_t* b = a.out_mrgb + 4 * size_t(to);
                b[0] = uint8_t((word >> 24) & 0x7fu);
                b[1] = uint8_t((word >> 16) & 0xffu);
                b[2] = uint8_t((word >> 8) & 0xffu);
                b[3] = uint8_t(word & 0xffu);
            }
            if (a.out_d2 != nullptr) store16(a.out_d2 + 2 * size_t(to), found[j] & 0xffffu);
            to++;
        }
    }
}

}  // namespace

hipError_t launch_distance_heads(const uint64_t* keys, uint32_t n, uint32_t shift, bool spread, uint64_t* part, uint64_t* out, hipStream_t s) {
    const dim3 grid(distance_head_blocks(n)), block(kDistanceThreads);
    if (out != nullptr)
        hipLaunchKernelGGL(distance_heads_kernel<true>, grid, block, 0, s, keys, n, shift, spread, part, out);
    else
        hipLaunchKernelGGL(distance_heads_kernel<false>, grid, block, 0, s, keys, n, shift, spread, part, out);
    return hipGetLastError();
}

hipError_t launch_distance(const DistanceArgs& a, hipStream_t s) {
    const dim3 grid(a.ntiles), block(kDistanceThreads);
    const bool invert = a.mode == kDistanceDepth || a.mode == kDistanceErode, emit = a.out_pos != nullptr;
    if (invert && emit)
        hipLaunchKernelGGL((distance_kernel<true, true>), grid, block, 0, s, a);
    else if (invert)
        hipLaunchKernelGGL((distance_kernel<true, false>), grid, block, 0, s, a);
    else if (emit)
        hipLaunchKernelGGL((distance_kernel<false, true>), grid, block, 0, s, a);
    else
        hipLaunchKernelGGL((distance_kernel<false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace vxrt
