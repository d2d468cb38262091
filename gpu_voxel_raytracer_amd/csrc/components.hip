// components.hip — device side of vxrt_components.h: the connected components of a voxel list.  The host side, which runs the launches
// and owns the scratch, is api_components.hip; the kernels' contract is in components.h and the argument in DESIGN.md §20.
//
//   keys          per entry: the path key at depth 15 and the entry's index
//   radix sort    device_build.hip: stable, so a run of equal keys keeps its entries in input order
//   heads         count / scan / write: the unique voxels in key order, each with its run's least input index
//   union         per unique voxel, its 3, 9 or 13 "lower" neighbours (every undirected pair once) by binary search in the unique
//                 keys; a union-find with parent[x] <= x joins them
//   flatten       a later launch: every voxel's root, the per-root minimum of the least input indices (or the anchor mark), and the
//                 number of roots by count / scan
//   scatter       a later launch: the result per sorted entry, written at the entry's input index
//   select        vxrt_detached_voxels_device only: count / scan / write of the flagged voxels in input (path) order
//
// Unique result: the forest's shape depends on the schedule, its roots do not (a tree's root is its least member, because parents
// never exceed their children, and the trees are the components once every pair has been joined).  What later launches read are
// roots and minima over a component, so every byte written to the caller is fixed by the rule.  Every output offset is a prefix sum.
// Bounds: every loop below is over a fixed count (kCompItems, 13 offsets, 16 key levels, 32 bisection steps) or follows parents
// strictly downward.  No workgroup waits for another, and the number of launches depends on n only.
#include "block_scan.h"
#include "components.h"
#include "device_build.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kCompThreads / 64;

// Unique result: no atomic, one store per entry.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void comp_keys_kernel(const int16_t* pos, uint32_t n, uint64_t* keys, uint32_t* vals) {
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i >= n) return;
        const uint32_t ux = uint32_t(int(pos[3 * i + 0]) + 32768), uy = uint32_t(int(pos[3 * i + 1]) + 32768),
                       uz = uint32_t(int(pos[3 * i + 2]) + 32768);
        keys[i] = path_key_of(ux, uy, uz, kCompDepth);
        vals[i] = uint32_t(i);
    }
}

__device__ __forceinline__ bool head_at(const uint64_t* keys, uint64_t i) { return i == 0 || keys[i] != keys[i - 1]; }

// Unique result: a count in thread order, no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void comp_heads_count_kernel(const uint64_t* keys, uint32_t n, uint64_t* part) {
    uint32_t mine = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i < n && head_at(keys, i)) mine++;
    }
    block_sum_to<kWaves>(mine, part + blockIdx.x);
}

// Unique result: every offset is the scanned part[block] plus a block prefix sum in entry order; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void comp_heads_write_kernel(const uint64_t* keys, const uint32_t* vals, uint32_t n, const uint64_t* part,
                                                                        uint64_t* ukeys, uint32_t* uhead, uint32_t* rank, uint32_t* parent,
                                                                        uint32_t* acc) {
    __shared__ uint32_t lds[kWaves];
    uint64_t at = part[blockIdx.x];   // the heads before this block
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        const bool ok = i < n;
        const bool head = ok && head_at(keys, i);
        uint32_t total;
        const uint32_t before = block_exclusive<uint32_t, kWaves>(head ? 1u : 0u, lds, &total);
        const uint32_t x = uint32_t(at + before);   // the heads before entry i; its own run's number when it is a head
        at += total;
        if (!ok) continue;
        if (head) {
            ukeys[x] = keys[i];
            uhead[x] = vals[i];
            parent[x] = x;
            acc[x] = kCompNone;
            rank[i] = x;
        } else {
            rank[i] = x - 1u;   // a head lies before it (entry 0 is one)
        }
    }
}

// ---- the union-find ------------------------------------------------------------------------------------------------------------
// parent[x] starts as x and only ever decreases: a root is hooked once, by a compare-and-swap from x to a smaller index, and after
// that the word moves by atomic minima to ancestors.  Every value a word ever held is therefore <= x, is != x only after x was
// hooked for good, and names a voxel of x's tree (trees merge and never split).  That is all find and unite rely on: a load here may
// return any value the word held since the launch began (MI355X: another CU's store need never reach this CU's L1), and a stale
// value is still a valid ancestor.  Only the read-modify-writes have to be coherent between workgroups.
__device__ __forceinline__ uint32_t parent_of(const uint32_t* parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // served by L2: staler values cost steps only
}

// A voxel of x's tree that looked like its root; the words passed on the way are lowered to their grandparents.
// Bound: x strictly decreases with every step (p != x means p < x), so at most x steps.
__device__ __forceinline__ uint32_t find_root(uint32_t* parent, uint32_t x) {
    uint32_t p = parent_of(parent, x);
    while (p != x) {
        const uint32_t g = parent_of(parent, p);
        if (g != p) atomicMin(parent + x, g);   // g < p < x: an ancestor whatever the order of arrival
        x = p;
        p = g;
    }
    return x;
}

// Joins the trees of a and b.  The hook validates through the compare-and-swap's returned value: it succeeds only on a word that
// still holds its own index, a true root, which then hangs under the smaller index b (b need not be a root any more: it is smaller
// and in another tree at that moment, since a tree's members are >= its root, so no cycle can form).  A failed hook returns the
// word's value, which is < a, and the retry goes on from there.  Bound: a + b strictly decreases with every retry.
__device__ __forceinline__ void unite(uint32_t* parent, uint32_t a, uint32_t b) {
    a = find_root(parent, a);
    b = find_root(parent, b);
    while (a != b) {
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = find_root(parent, old);
    }
}

// the "lower" half of the 26 offsets (the first nonzero component is -1), by the number of axes that differ: 3, then 6, then 4
__device__ const int8_t kLower[13][3] = {{-1, 0, 0}, {0, -1, 0}, {0, 0, -1},
                                         {-1, -1, 0}, {-1, 1, 0}, {-1, 0, -1}, {-1, 0, 1}, {0, -1, -1}, {0, -1, 1},
                                         {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

// Unique result: see the head of the file; the atomics are the hook's compare-and-swap and the lowering minimum.  Bounds: kCompItems
// rounds, at most 13 offsets, 32 bisection steps, find_root's and unite's.  Coordinates do not wrap: a neighbour outside [0, 2^16)
// is skipped.
__global__ __launch_bounds__(kCompThreads) void comp_union_kernel(const uint64_t* ukeys, uint32_t m, uint32_t offsets, uint32_t* parent) {
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i >= m) return;
        const uint32_t x = uint32_t(i);
        uint32_t u[3];
        cell_of(ukeys[x], u);
#pragma unroll 1
        for (uint32_t k = 0; k < offsets; k++) {
            const uint32_t vx = u[0] + uint32_t(int(kLower[k][0])), vy = u[1] + uint32_t(int(kLower[k][1])), vz = u[2] + uint32_t(int(kLower[k][2]));
            if ((vx | vy | vz) > 0xffffu) continue;
            const uint64_t want = path_key_of(vx, vy, vz, kCompDepth);
            uint32_t lo = 0, hi = m;   // the first unique key >= want
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (ukeys[mid] < want) lo = mid + 1u; else hi = mid;
            }
            if (lo < m && ukeys[lo] == want) unite(parent, x, lo);
        }
    }
}

// A launch after the union, so parent[] is final and plain loads read it.  Unique result: a root is the least voxel of its
// component; the atomic is a minimum, whose fixed point does not depend on the order; the root count is a sum in thread order.
// Bounds: kCompItems rounds; the walk to the root strictly decreases.
__global__ __launch_bounds__(kCompThreads) void comp_flatten_kernel(const uint64_t* ukeys, const uint32_t* uhead, const uint32_t* parent, uint32_t m,
                                                                    const CompBox box, uint32_t* comp, uint32_t* acc, uint64_t* part) {
    uint32_t roots = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i >= m) break;
        const uint32_t x = uint32_t(i);
        uint32_t r = x, p = parent[r];
        while (p != r) { r = p; p = parent[r]; }
        comp[x] = r;
        if (r == x) roots++;
        uint32_t v = uhead[x];
        if (box.on) {
            uint32_t u[3];
            cell_of(ukeys[x], u);
            bool in = true;
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                const int32_t c = int32_t(u[ax]) - 32768;
                in = in && c >= box.lo[ax] && c < box.hi[ax];
            }
            v = in ? 0u : kCompNone;
        }
        if (v != kCompNone) atomicMin(acc + r, v);
    }
    block_sum_to<kWaves>(roots, part + blockIdx.x);
}

// A launch after the flatten, so comp[] and acc[] are final.  Unique result: vals is a permutation of the indices, so every word of
// out is written once; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void comp_scatter_kernel(const uint32_t* vals, const uint32_t* rank, uint32_t n, const uint32_t* comp,
                                                                    const uint32_t* acc, uint32_t detached, uint32_t* out) {
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i >= n) return;
        const uint32_t v = acc[comp[rank[i]]];
        out[vals[i]] = detached ? (v != 0u ? 1u : 0u) : v;
    }
}

// Unique result: a count in thread order, no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void comp_select_count_kernel(const uint32_t* flag, uint32_t n, uint64_t* part) {
    uint32_t mine = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i < n && flag[i] != 0u) mine++;
    }
    block_sum_to<kWaves>(mine, part + blockIdx.x);
}

// Unique result: every offset is the scanned part[block] plus a block prefix sum in entry order; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void comp_select_write_kernel(const uint32_t* flag, uint32_t n, const uint64_t* part, const int16_t* src_pos,
                                                                         const uint32_t* src_mrgb, int16_t* dst_pos, uint32_t* dst_mrgb) {
    __shared__ uint32_t lds[kWaves];
    uint64_t at = part[blockIdx.x];
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        const bool keep = i < n && flag[i] != 0u;
        uint32_t total;
        const uint64_t o = at + block_exclusive<uint32_t, kWaves>(keep ? 1u : 0u, lds, &total);
        at += total;
        if (keep) {
            dst_pos[3 * o + 0] = src_pos[3 * i + 0];
            dst_pos[3 * o + 1] = src_pos[3 * i + 1];
            dst_pos[3 * o + 2] = src_pos[3 * i + 2];
            dst_mrgb[o] = src_mrgb[i];
        }
    }
}

}  // namespace

hipError_t components_keys(const int16_t* pos, uint32_t n, uint64_t* keys, uint32_t* vals, hipStream_t s) {
    hipLaunchKernelGGL(comp_keys_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, pos, n, keys, vals);
    return hipGetLastError();
}

hipError_t components_heads_count(const uint64_t* keys, uint32_t n, uint64_t* part, hipStream_t s) {
    hipLaunchKernelGGL(comp_heads_count_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, keys, n, part);
    return hipGetLastError();
}

hipError_t components_heads_write(const uint64_t* keys, const uint32_t* vals, uint32_t n, const uint64_t* part, uint64_t* ukeys, uint32_t* uhead,
                                  uint32_t* rank, uint32_t* parent, uint32_t* acc, hipStream_t s) {
    hipLaunchKernelGGL(comp_heads_write_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, keys, vals, n, part, ukeys, uhead, rank, parent, acc);
    return hipGetLastError();
}

hipError_t components_union(const uint64_t* ukeys, uint32_t m, uint32_t axes, uint32_t* parent, hipStream_t s) {
    const uint32_t offsets = axes == 1u ? 3u : axes == 2u ? 9u : 13u;
    hipLaunchKernelGGL(comp_union_kernel, dim3(comp_blocks(m)), dim3(kCompThreads), 0, s, ukeys, m, offsets, parent);
    return hipGetLastError();
}

hipError_t components_flatten(const uint64_t* ukeys, const uint32_t* uhead, const uint32_t* parent, uint32_t m, CompBox box, uint32_t* comp,
                              uint32_t* acc, uint64_t* part, hipStream_t s) {
    hipLaunchKernelGGL(comp_flatten_kernel, dim3(comp_blocks(m)), dim3(kCompThreads), 0, s, ukeys, uhead, parent, m, box, comp, acc, part);
    return hipGetLastError();
}

hipError_t components_scatter(const uint32_t* vals, const uint32_t* rank, uint32_t n, const uint32_t* comp, const uint32_t* acc, uint32_t detached,
                              uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(comp_scatter_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, vals, rank, n, comp, acc, detached, out);
    return hipGetLastError();
}

hipError_t components_select_count(const uint32_t* flag, uint32_t n, uint64_t* part, hipStream_t s) {
    hipLaunchKernelGGL(comp_select_count_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, flag, n, part);
    return hipGetLastError();
}

hipError_t components_select_write(const uint32_t* flag, uint32_t n, const uint64_t* part, const int16_t* src_pos, const uint32_t* src_mrgb,
                                   int16_t* dst_pos, uint32_t* dst_mrgb, hipStream_t s) {
    hipLaunchKernelGGL(comp_select_write_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, flag, n, part, src_pos, src_mrgb, dst_pos, dst_mrgb);
    return hipGetLastError();
}

}  // namespace vxrt
