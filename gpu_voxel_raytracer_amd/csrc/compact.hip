// compact.hip — device side of vxrt_compact.h: the scene's live tree written into a second pair of arrays in the layout of a fresh
// build, one node level at a time over the whole device.  The host side, which runs the levels and swaps the arrays in, is
// api_compact.hip; the scheme is in compact.h.
//
// A thread takes kCompactItems consecutive entries of the level: 64 bytes of the new record array, read and written as four 16-byte
// accesses where the whole group belongs to the level (every group but a level's first and last), entry by entry otherwise.  The
// fetch of the old records in compact_count is the only irregular access; a node's children are one run of up to 64 bytes in the old
// array, so compact_expand hands them out by index without touching them.
#include "block_scan.h"
#include "compact.h"

namespace vxrt {
namespace {

// A thread's group of entries: `first` = index into dst of the group's first entry (even), bit j of `live` = entry first + j belongs
// to the level.  Groups are numbered from the even index at or below a.start.
struct Group {
    uint64_t first;
    uint32_t live;
};

__device__ __forceinline__ Group group_of(const CompactLevel& a) {
    const uint64_t lo = a.start, hi = uint64_t(a.start) + a.n;
    Group g;
    g.first = (lo & ~uint64_t(1)) + (uint64_t(blockIdx.x) * kCompactThreads + threadIdx.x) * kCompactItems;
    g.live = 0;
#pragma unroll
    for (uint32_t j = 0; j < kCompactItems; j++)
        if (g.first + j >= lo && g.first + j < hi) g.live |= 1u << j;
    return g;
}

__device__ __forceinline__ void load_group(const CompactLevel& a, const Group& g, SvoRecord (&r)[kCompactItems]) {
    if (g.live == 0xffu) {
        const uint4* p = reinterpret_cast<const uint4*>(a.dst + g.first);
#pragma unroll
        for (uint32_t j = 0; j < kCompactItems; j += 2) {
            const uint4 v = p[j / 2];
            r[j] = SvoRecord{v.x, v.y};
            r[j + 1] = SvoRecord{v.z, v.w};
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kCompactItems; j++) {
            r[j] = SvoRecord{0u, 0u};
            if (g.live >> j & 1u) {
                const uint2 v = *reinterpret_cast<const uint2*>(a.dst + g.first + j);
                r[j] = SvoRecord{v.x, v.y};
            }
        }
    }
}

__device__ __forceinline__ void store_group(const CompactLevel& a, const Group& g, const SvoRecord (&r)[kCompactItems]) {
    if (g.live == 0xffu) {
        uint4* p = reinterpret_cast<uint4*>(a.dst + g.first);
#pragma unroll
        for (uint32_t j = 0; j < kCompactItems; j += 2) p[j / 2] = make_uint4(r[j].masks, r[j].base, r[j + 1].masks, r[j + 1].base);
    } else {
#pragma unroll
        for (uint32_t j = 0; j < kCompactItems; j++)
            if (g.live >> j & 1u) *reinterpret_cast<uint2*>(a.dst + g.first + j) = make_uint2(r[j].masks, r[j].base);
    }
}

// the slots a node of this level holds: children, or leaf words at the leaf parents
__device__ __forceinline__ uint32_t slots_of(const CompactLevel& a, const SvoRecord& r) {
    return uint32_t(__popc(a.leaf ? (r.masks >> 8) & 0xffu : r.masks & 0xffu));
}

__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(const CompactLevel a) {
    __shared__ uint32_t lds[kCompactThreads / 64];
    const Group g = group_of(a);
    SvoRecord r[kCompactItems];
    load_group(a, g, r);
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kCompactItems; j++) {
        // {0, index in the old array} -> the old record; an index past the records in use reads as a node without slots (the host
        // then finds fewer records than the context counts and refuses)
        SvoRecord old{0u, 0u};
        if ((g.live >> j & 1u) && r[j].base < a.src_count) {
            const uint2 v = *reinterpret_cast<const uint2*>(a.src + r[j].base);
            old = SvoRecord{v.x, v.y};
        }
        r[j] = old;
        sum += slots_of(a, old);
    }
    store_group(a, g, r);
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < kCompactThreads / 64; w++) all += lds[w];
        a.part[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kCompactThreads) void compact_expand_kernel(const CompactLevel a) {
    __shared__ uint32_t lds[kCompactThreads / 64];
    const Group g = group_of(a);
    SvoRecord r[kCompactItems];
    load_group(a, g, r);
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kCompactItems; j++) mine += slots_of(a, r[j]);   // entries outside the level read as {0, 0}
    uint32_t total;
    uint64_t o = a.part[blockIdx.x] + block_exclusive<uint32_t, kCompactThreads / 64>(mine, lds, &total);
    const uint64_t below = uint64_t(a.start) + a.n;   // where the next level starts
#pragma unroll
    for (uint32_t j = 0; j < kCompactItems; j++) {
        const uint32_t k = slots_of(a, r[j]), from = r[j].base;
        if (a.leaf) {
#pragma unroll
            for (uint32_t i = 0; i < 8; i++)
                if (i < k && o + i < a.dst_leaf_count) a.dst_leaves[o + i] = uint64_t(from) + i < a.src_leaf_count ? a.src_leaves[from + i] : 0;
            r[j].base = uint32_t(o);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 8; i++)
                if (i < k && below + o + i < a.dst_count) *reinterpret_cast<uint2*>(a.dst + below + o + i) = make_uint2(0u, from + i);
            r[j].base = uint32_t(below + o);
        }
        o += k;
    }
    store_group(a, g, r);
}

}  // namespace

hipError_t launch_compact_count(const CompactLevel& a, hipStream_t s) {
    hipLaunchKernelGGL(compact_count_kernel, dim3(compact_blocks(a.start, a.n)), dim3(kCompactThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_compact_expand(const CompactLevel& a, hipStream_t s) {
    hipLaunchKernelGGL(compact_expand_kernel, dim3(compact_blocks(a.start, a.n)), dim3(kCompactThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace vxrt
