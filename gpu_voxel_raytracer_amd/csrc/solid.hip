// solid.hip — device side of vxrt_solid.h: the interior cells of a closed triangle mesh, by crossing parity along z, as path keys
// and leaf words ready for the list builder's sort and dedupe (device_build.hip: sort_unique_list).  The host side is api_solid.hip;
// the snapped triangles come from voxelize.hip's setup pass; the rule, in exact integer arithmetic, is DESIGN.md §18.
//
//   columns   a thread per triangle: its z-columns (the cells (x, y) whose centre lies inside its bounds; none for a triangle that
//             is vertical or thinner than the gap between two centres) -> the block's exclusive offsets -> zoff[t], part[block]
//   spread    zoff[t] += part[block of t] after the scan; zoff[n_tris] = the total (the same kernel spreads the pairs' offsets)
//   cross     a thread per (triangle, column) item.  A triangle can have no column, so 256 consecutive items may span any number of
//             triangles: each thread binary-searches the global offsets for the last triangle that starts at or before its item.
//             Rule 2 decides whether the column's centre is under the triangle, rule 3 where the plane crosses it.  Counting: the
//             block's crossings -> part[block].  Emitting: the crossing's key at part[block] + the thread's exclusive offset.
//   pairs     the keys sorted: a thread per pair (2j, 2j + 1).  A closed mesh has an even count in every column, so every column
//             starts at an even index and a pair shares its column; the first pair that does not marks the first odd column (a
//             minimum over the pair index).  The pair's interior length k_1 - k_0 -> the block's exclusive offsets, as above.
//   fill      a thread per interior cell: its pair by the same search in the pairs' offsets (lengths of 0 are common), the cell
//             k_0 + the thread's rank in the pair -> the path key and the fill word
// 256 threads, no atomics: every position is a prefix sum in a fixed order.
#include <string>

#include "block_scan.h"
#include "ctx.h"
#include "device_build.h"
#include "solid.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kVoxThreads / 64;
constexpr uint32_t kNone = 0xffffffffu;

struct Tri {
    int q[9];       // [3 * vertex + axis]
};

__device__ __forceinline__ Tri load_tri(const VoxTri* tq, uint32_t t) {
    const uint4* src = reinterpret_cast<const uint4*>(tq + t);
    const uint4 a = src[0], b = src[1], c = src[2];
    return Tri{{int(a.x), int(a.y), int(a.z), int(a.w), int(b.x), int(b.y), int(b.z), int(b.w), int(c.x)}};
}

// n_z of n = e0 x e1, e0 = q_1 - q_0, e1 = q_2 - q_1
__device__ __forceinline__ int64_t normal_z(const Tri& t) {
    return wmul(t.q[3] - t.q[0], t.q[7] - t.q[4]) - wmul(t.q[4] - t.q[1], t.q[6] - t.q[3]);
}

// rule 1: the columns [*x0, *x0 + *nx) x [*y0, *y0 + *ny) whose centre 16 c + 8 lies in [lo, hi] on both axes
__device__ __forceinline__ uint64_t z_columns(const Tri& t, int* x0, int* nx, int* y0, int* ny) {
    *x0 = (min3(t.q[0], t.q[3], t.q[6]) + 7) >> 4;                      // ceil((lo - 8) / 16)
    *nx = max(((max3(t.q[0], t.q[3], t.q[6]) - 8) >> 4) - *x0 + 1, 0);  // floor((hi - 8) / 16)
    *y0 = (min3(t.q[1], t.q[4], t.q[7]) + 7) >> 4;
    *ny = max(((max3(t.q[1], t.q[4], t.q[7]) - 8) >> 4) - *y0 + 1, 0);
    return normal_z(t) == 0 ? 0ull : uint64_t(*nx) * uint64_t(*ny);
}

// rule 2 for one edge a -> b and the point p, all in the xy-plane
__device__ __forceinline__ bool edge_counts(int ax, int ay, int bx, int by, int px, int py) {
    if ((ay <= py) == (by <= py)) return false;
    const bool up = ay <= py;       // l = a, u = b
    const int lx = up ? ax : bx, ly = up ? ay : by, ux = up ? bx : ax, uy = up ? by : ay;
    return wmul(ux - lx, py - ly) - wmul(px - lx, uy - ly) > 0;
}

// off[0 .. n]: ascending, off[0] == 0, g < off[n].  The owner of g is the last entry at or before it, which is the one that is not
// empty: off[owner] <= g < off[owner + 1].
__device__ __forceinline__ uint32_t find_owner(const uint64_t* off, uint32_t n, uint64_t g) {
    uint32_t lo = 0;
    for (uint32_t hi = n - 1; lo < hi;) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kVoxThreads) void solid_columns_kernel(const VoxTri* tq, uint32_t n_tris, uint64_t* zoff, uint64_t* part) {
    __shared__ uint64_t lds[kWaves];
    const uint32_t t = blockIdx.x * kVoxThreads + threadIdx.x;
    uint64_t columns = 0;
    if (t < n_tris) {
        int x0, nx, y0, ny;
        columns = z_columns(load_tri(tq, t), &x0, &nx, &y0, &ny);
    }
    uint64_t total;
    const uint64_t before = block_exclusive<uint64_t, kWaves>(columns, lds, &total);
    if (t < n_tris) zoff[t] = before;
    if (threadIdx.x == 0) part[blockIdx.x] = total;
}

// off[i]: within its block -> over all n entries; off[n] = the total
__global__ __launch_bounds__(kVoxThreads) void solid_spread_kernel(uint64_t* off, const uint64_t* part, uint32_t n, uint32_t blocks) {
    const uint64_t i = uint64_t(blockIdx.x) * kVoxThreads + threadIdx.x;
    if (i < n) off[i] += part[blockIdx.x];
    else if (i == n) off[i] = part[blocks];
}

// kEmit false: part[block] = the block's crossings.  kEmit true: part[block] is the crossings before the block.
template <bool kEmit>
__global__ __launch_bounds__(kVoxThreads) void solid_cross_kernel(const VoxTri* tq, const uint64_t* zoff, uint32_t n_tris, uint32_t columns, uint64_t* part,
                                                                   SolidKeying keying, uint64_t* keys) {
    __shared__ uint64_t lds[kWaves];
    const uint64_t g = uint64_t(blockIdx.x) * kVoxThreads + threadIdx.x;
    bool under = false;
    uint64_t key = 0;
    if (g < columns) {
        const uint32_t t = find_owner(zoff, n_tris, g);
        const Tri tri = load_tri(tq, t);
        int x0, nx, y0, ny;
        (void)z_columns(tri, &x0, &nx, &y0, &ny);
        const uint32_t k = uint32_t(g - zoff[t]);
        const int x = x0 + int(k % uint32_t(nx)), y = y0 + int(k / uint32_t(nx));
        const int px = 16 * x + 8, py = 16 * y + 8;
        const int* q = tri.q;
        under = edge_counts(q[0], q[1], q[3], q[4], px, py) != edge_counts(q[3], q[4], q[6], q[7], px, py) !=
                edge_counts(q[6], q[7], q[0], q[1], px, py);
        if (kEmit && under) {
            // rule 3: the least cell whose centre lies strictly above the plane, floor(-sigma A / (16 |n_z|)) + 1
            const int e0[3] = {q[3] - q[0], q[4] - q[1], q[5] - q[2]}, e1[3] = {q[6] - q[3], q[7] - q[4], q[8] - q[5]};
            const int64_t n0 = wmul(e0[1], e1[2]) - wmul(e0[2], e1[1]), n1 = wmul(e0[2], e1[0]) - wmul(e0[0], e1[2]),
                          n2 = wmul(e0[0], e1[1]) - wmul(e0[1], e1[0]);
            const int64_t a = n0 * (px - q[0]) + n1 * (py - q[1]) + n2 * (8 - q[2]);      // |a| < 3 * 2^61
            const int64_t num = n2 > 0 ? -a : a, den = 16 * (n2 > 0 ? n2 : -n2);
            int64_t fl = num / den;
            if (num - fl * den < 0) fl--;       // the division truncates; the rule wants the floor
            const int cell = int(fl) + 1;
            key = uint64_t(uint32_t(x - keying.lo[0])) << (keying.by + keying.bz) | uint64_t(uint32_t(y - keying.lo[1])) << keying.bz |
                  uint64_t(uint32_t(cell - keying.lo[2]));
        }
    }
    uint64_t total;
    const uint64_t before = block_exclusive<uint64_t, kWaves>(under ? 1ull : 0ull, lds, &total);
    if (!kEmit) {
        if (threadIdx.x == 0) part[blockIdx.x] = total;
        return;
    }
    if (under) keys[part[blockIdx.x] + before] = key;
}

// the block's least v -> *out (thread 0 writes)
__device__ __forceinline__ void block_min(uint32_t v, uint32_t* out) {
    __shared__ uint32_t lds[kWaves];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, uint32_t(__shfl_xor(int(v), off, 64)));
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kWaves; w++) v = min(v, lds[w]);
        *out = v;
    }
}

__global__ __launch_bounds__(kVoxThreads) void solid_pairs_kernel(const uint64_t* keys, uint32_t pairs, uint32_t bz, uint64_t* loff, uint64_t* part,
                                                                   uint32_t* split) {
    __shared__ uint64_t lds[kWaves];
    const uint32_t j = blockIdx.x * kVoxThreads + threadIdx.x;
    uint64_t length = 0;
    uint32_t bad = kNone;
    if (j < pairs) {
        const uint64_t a = keys[2 * size_t(j)], b = keys[2 * size_t(j) + 1];
        if ((a >> bz) == (b >> bz)) length = b - a;      // the same column: k_1 - k_0 >= 0, the keys are sorted
        else bad = j;
    }
    uint64_t total;
    const uint64_t before = block_exclusive<uint64_t, kWaves>(length, lds, &total);
    if (j < pairs) loff[j] = before;
    if (threadIdx.x == 0) part[blockIdx.x] = total;
    block_min(bad, split + blockIdx.x);
}

__global__ __launch_bounds__(kVoxThreads) void solid_split_kernel(uint32_t* split, uint32_t blocks) {
    uint32_t v = kNone;
    for (uint32_t k = threadIdx.x; k < blocks; k += kVoxThreads) v = min(v, split[k]);
    block_min(v, split + blocks);
}

// one thread: the column of keys[at] and how many of the n sorted keys lie in it
__global__ void solid_open_kernel(const uint64_t* keys, uint32_t n, uint32_t at, SolidKeying keying, SolidOpen* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const uint64_t col = keys[at] >> keying.bz;
    uint32_t first = 0, past = n;       // the first key of the column; the first key past it
    for (uint32_t hi = at; first < hi;) {
        const uint32_t mid = first + (hi - first) / 2;
        if ((keys[mid] >> keying.bz) < col) first = mid + 1; else hi = mid;
    }
    for (uint32_t lo = at + 1; lo < past;) {
        const uint32_t mid = lo + (past - lo) / 2;
        if ((keys[mid] >> keying.bz) > col) past = mid; else lo = mid + 1;
    }
    SolidOpen r;
    r.x = int32_t(col >> keying.by) + keying.lo[0];
    r.y = int32_t(col & ((uint64_t(1) << keying.by) - 1u)) + keying.lo[1];
    r.crossings = past - first;
    r.pad = 0u;
    *out = r;
}

__global__ __launch_bounds__(kVoxThreads) void solid_fill_kernel(const uint64_t* keys, const uint64_t* loff, uint32_t pairs, uint32_t cells,
                                                                  SolidKeying keying, uint32_t depth, uint32_t word, uint64_t* out_keys,
                                                                  uint32_t* out_vals) {
    const uint64_t i = uint64_t(blockIdx.x) * kVoxThreads + threadIdx.x;
    if (i >= cells) return;
    const uint32_t j = find_owner(loff, pairs, i);
    const uint64_t a = keys[2 * size_t(j)], col = a >> keying.bz;
    const int x = int(col >> keying.by) + keying.lo[0], y = int(col & ((uint64_t(1) << keying.by) - 1u)) + keying.lo[1];
    const int z = int(a & ((uint64_t(1) << keying.bz) - 1u)) + keying.lo[2] + int(i - loff[j]);
    const int half = 1 << depth;
    out_keys[i] = path_key_of(uint32_t(x + half), uint32_t(y + half), uint32_t(z + half), depth);
    if (out_vals) out_vals[i] = word;
}

uint32_t bits_for(uint32_t v) {      // the least b with v < 2^b
    uint32_t b = 0;
    while ((uint64_t(1) << b) <= v) b++;
    return b;
}

}  // namespace

SolidKeying solid_keying(const MeshSummary& ms) {
    SolidKeying k;
    for (int ax = 0; ax < 3; ax++) k.lo[ax] = ms.lo[ax];
    const uint32_t bx = bits_for(uint32_t(ms.hi[0] - ms.lo[0]));
    k.by = bits_for(uint32_t(ms.hi[1] - ms.lo[1]));
    k.bz = bits_for(uint32_t(ms.hi[2] - ms.lo[2]) + 1u);      // a crossing may lie one cell above the highest candidate
    k.bits = bx + k.by + k.bz;
    return k;
}

int solid_columns(const VoxTri* tq, uint32_t n_tris, uint64_t* zoff, uint64_t* part, hipStream_t s, uint64_t* columns) {
    const uint32_t blocks = vox_blocks(n_tris);
    hipLaunchKernelGGL(solid_columns_kernel, dim3(blocks), dim3(kVoxThreads), 0, s, tq, n_tris, zoff, part);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_exclusive_scan(part, blocks, s));
    hipLaunchKernelGGL(solid_spread_kernel, dim3(vox_blocks(uint64_t(n_tris) + 1)), dim3(kVoxThreads), 0, s, zoff, part, n_tris, blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(columns, part + blocks, sizeof *columns, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

int solid_count(const VoxTri* tq, const uint64_t* zoff, uint32_t n_tris, uint32_t columns, uint64_t* part, hipStream_t s, uint64_t* crossings) {
    const uint32_t blocks = vox_blocks(columns);
    hipLaunchKernelGGL(solid_cross_kernel<false>, dim3(blocks), dim3(kVoxThreads), 0, s, tq, zoff, n_tris, columns, part, SolidKeying{}, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_exclusive_scan(part, blocks, s));
    HIP_TRY(hipMemcpyAsync(crossings, part + blocks, sizeof *crossings, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

hipError_t solid_emit(const VoxTri* tq, const uint64_t* zoff, uint32_t n_tris, uint32_t columns, const uint64_t* part, SolidKeying keying,
                      uint64_t* keys, hipStream_t s) {
    hipLaunchKernelGGL(solid_cross_kernel<true>, dim3(vox_blocks(columns)), dim3(kVoxThreads), 0, s, tq, zoff, n_tris, columns,
                       const_cast<uint64_t*>(part), keying, keys);
    return hipGetLastError();
}

int solid_pairs(const uint64_t* keys, uint32_t crossings, SolidKeying keying, uint64_t* loff, uint64_t* part, const char* who, hipStream_t s,
                bool* closed, SolidOpen* open, uint64_t* cells) {
    const uint32_t pairs = crossings / 2u, blocks = vox_blocks(pairs);
    ScratchBuffer split, found;
    if (int rc = alloc_scratch(&split, (size_t(blocks) + 1) * sizeof(uint32_t), who, "the pairs' columns")) return rc;
    if (int rc = alloc_scratch(&found, sizeof(SolidOpen), who, "the open column")) return rc;
    uint32_t first_split = kNone;
    *cells = 0;
    if (pairs != 0u) {
        hipLaunchKernelGGL(solid_pairs_kernel, dim3(blocks), dim3(kVoxThreads), 0, s, keys, pairs, keying.bz, loff, part, split.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(solid_split_kernel, dim3(1), dim3(kVoxThreads), 0, s, split.as<uint32_t>(), blocks);
        HIP_TRY(hipGetLastError());
        HIP_TRY(launch_exclusive_scan(part, blocks, s));
        hipLaunchKernelGGL(solid_spread_kernel, dim3(vox_blocks(uint64_t(pairs) + 1)), dim3(kVoxThreads), 0, s, loff, part, pairs, blocks);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&first_split, split.as<uint32_t>() + blocks, sizeof first_split, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(cells, part + blocks, sizeof *cells, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *closed = first_split == kNone && (crossings & 1u) == 0u;
    if (*closed) return VXRT_OK;
    // the first pair that spans two columns starts in the first odd column; without one, the last crossing is alone in its column
    const uint32_t at = first_split != kNone ? 2u * first_split : crossings - 1u;
    hipLaunchKernelGGL(solid_open_kernel, dim3(1), dim3(64), 0, s, keys, crossings, at, keying, found.as<SolidOpen>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(open, found.get(), sizeof *open, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

hipError_t solid_fill(const uint64_t* keys, const uint64_t* loff, uint32_t pairs, uint32_t cells, SolidKeying keying, uint32_t depth,
                      uint32_t word, uint64_t* out_keys, uint32_t* out_vals, hipStream_t s) {
    hipLaunchKernelGGL(solid_fill_kernel, dim3(vox_blocks(cells)), dim3(kVoxThreads), 0, s, keys, loff, pairs, cells, keying, depth, word, out_keys,
                       out_vals);
    return hipGetLastError();
}

}  // namespace vxrt
