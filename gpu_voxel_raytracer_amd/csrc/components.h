// components.h — what api_components.hip (host side of vxrt_components.h) and components.hip (its kernels) share.  DESIGN.md §20.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ctx.h"
#include "device_build.h"

namespace vxrt {

// Every kernel here runs blocks of kCompThreads threads over kCompSpan consecutive entries each, kCompItems rounds of one entry per
// thread (the layout of extract.hip), so a grid has comp_blocks(n) <= 2^21 blocks for n < 2^32.  Every output offset is a prefix
// sum over that numbering: per-block counts -> launch_exclusive_scan (device_build.h) -> the write pass.
constexpr uint32_t kCompThreads = 256;
constexpr uint32_t kCompItems = 8;
constexpr uint32_t kCompSpan = kCompThreads * kCompItems;
constexpr uint32_t kCompDepth = 15;                        // every int16 position has a path key at this depth ...
constexpr uint32_t kCompKeyBits = 3u * (kCompDepth + 1u);  // ... of 48 bits
constexpr uint32_t kCompNone = 0xffffffffu;

inline uint32_t comp_blocks(uint64_t n) { return uint32_t((n + kCompSpan - 1) / kCompSpan); }

// this block's round-j entry of this thread (< 2^32 + kCompSpan)
__device__ __forceinline__ uint64_t entry_of(uint32_t j) { return uint64_t(blockIdx.x) * kCompSpan + j * kCompThreads + threadIdx.x; }

// a depth-15 path key -> u = p + 2^15 per axis (the inverse of path_key_of)
__device__ __forceinline__ void cell_of(uint64_t key, uint32_t u[3]) {
    u[0] = u[1] = u[2] = 0;
#pragma unroll
    for (uint32_t k = 0; k <= kCompDepth; k++) {
        const uint32_t t = uint32_t(key >> (3u * k)) & 7u;
        u[0] |= (t >> 2) << k;
        u[1] |= ((t >> 1) & 1u) << k;
        u[2] |= (t & 1u) << k;
    }
}

// The half-open anchor box of vxrt_detached_voxels_device; on == 0: there is none (vxrt_label_components_device).
struct CompBox {
    int32_t lo[3], hi[3];
    uint32_t on;
};

// keys[i] = the path key of pos[i] at depth 15 (device_build.h: path_key_of), vals[i] = i.  pos may have any alignment.
hipError_t components_keys(const int16_t* pos, uint32_t n, uint64_t* keys, uint32_t* vals, hipStream_t s);

// Over the n sorted keys: part[b] = the run heads (an entry whose key differs from its predecessor's) among block b's entries.
hipError_t components_heads_count(const uint64_t* keys, uint32_t n, uint64_t* part, hipStream_t s);

// part scanned.  Run head number x (m of them, in key order): ukeys[x] = its key, uhead[x] = its value (the sort is stable, so the
// least input index of the run), parent[x] = x, acc[x] = kCompNone.  Every sorted entry i: rank[i] = the number of its run.
hipError_t components_heads_write(const uint64_t* keys, const uint32_t* vals, uint32_t n, const uint64_t* part, uint64_t* ukeys,
                                  uint32_t* uhead, uint32_t* rank, uint32_t* parent, uint32_t* acc, hipStream_t s);

// The union-find over the m unique voxels: every pair that differs by at most 1 on every axis and on at most `axes` (1, 2, 3) axes
// is joined.  On return (of the launch) parent[] is a forest with parent[x] <= x whose trees are the components.
hipError_t components_union(const uint64_t* ukeys, uint32_t m, uint32_t axes, uint32_t* parent, hipStream_t s);

// comp[x] = the root of x (the least unique voxel of its component); acc[comp[x]] = the least uhead of the component (box.on == 0)
// or 0 when a voxel of the component lies in the box (box.on != 0; kCompNone otherwise); part[b] = the roots in block b.
hipError_t components_flatten(const uint64_t* ukeys, const uint32_t* uhead, const uint32_t* parent, uint32_t m, CompBox box, uint32_t* comp,
                              uint32_t* acc, uint64_t* part, hipStream_t s);

// Back to input order, over the n sorted entries: out[vals[i]] = acc[comp[rank[i]]], or with `detached` 1 where that is not 0, else 0.
hipError_t components_scatter(const uint32_t* vals, const uint32_t* rank, uint32_t n, const uint32_t* comp, const uint32_t* acc,
                              uint32_t detached, uint32_t* out, hipStream_t s);

// The selection of the flagged entries of a list of n: part[b] = the flags set in block b; then, part scanned, entry i with flag[i]
// set goes to the offset of the flags before it: its position (3 int16; src and dst 2-byte aligned) and mrgb word (4-byte aligned).
hipError_t components_select_count(const uint32_t* flag, uint32_t n, uint64_t* part, hipStream_t s);
hipError_t components_select_write(const uint32_t* flag, uint32_t n, const uint64_t* part, const int16_t* src_pos, const uint32_t* src_mrgb,
                                   int16_t* dst_pos, uint32_t* dst_mrgb, hipStream_t s);

// ---- api_components.hip: the labelling that vxrt_components.h's calls and vxrt_pieces.h's (api_pieces.hip) share ----------------------
// The scratch of one labelling and what it leaves: for sorted entry i, sorted[i] is its input index and rank[i] its unique voxel;
// for unique voxel x in key order, ukeys[x] is its path key, uhead[x] the least input index at its position, comp[x] its root and
// acc[comp[x]] the component's value (components_flatten); part holds the flatten's root counts, scanned: part[b] = the roots before
// block b, part[comp_blocks(unique)] = components.
struct Labelling {
    KeySort ls;          // keys and input indices, double-buffered, and the sort's counts
    ScratchBuffer uhead, parent, comp, acc, part;
    const uint64_t* ukeys = nullptr;
    const uint32_t* sorted = nullptr;
    const uint32_t* rank = nullptr;
    uint32_t unique = 0;
    uint64_t components = 0;
};

// About 40 bytes per entry, all of it allocated before the first launch.
int alloc_labelling(size_t n, const char* who, Labelling* l);

// pos[0 .. n), 0 < n < 2^32, read on s -> *l.  axes: 1, 2 or 3.  Waits for the two counts.
int label_list(const int16_t* pos, uint32_t n, uint32_t axes, const CompBox& box, hipStream_t s, Labelling* l);

// 6, 18, 26 -> the axes on which two neighbours may differ; anything else -> 0
uint32_t axes_of(uint32_t connectivity);

}  // namespace vxrt
