// compact.h — what api_compact.hip (host side of vxrt_compact.h) and compact.hip (its kernels) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace vxrt {

// The relayout is level-synchronous from the root, like the decode (extract.h): node level l has n nodes in breadth-first order and
// takes the entries [start, start + n) of the NEW record array; its children take [start + n, ...) in the same order, slots ascending.
// No frontier buffer: until a level is expanded, its entries of the new array carry {0, index of the node's record in the old array}.
// Each level is three launches over its entries, in blocks of kCompactSpan:
//   compact_count   every entry fetches its old record — the one irregular read — and keeps it, {masks, old base}, in place;
//                   per block: the number of children (leaf words at the leaf parents' level) -> part[block]
//   exclusive_scan  one workgroup: part[] -> its exclusive prefix sum in place, the total -> part[blocks] (device_build.h)
//   compact_expand  every entry becomes the final record {masks, start + n + offset} ({masks, offset} at the leaf parents); child j
//                   of a node gets {0, old base + j} (children are contiguous in the old array, whatever block they live in); at
//                   the leaf parents the leaf words old base + j are copied to offset + j
// Every position is a prefix sum in breadth-first order and nothing is decided by an atomic: two calls write the same bytes, and
// those are the bytes of api_scene.hip's flatten_svo.
constexpr uint32_t kCompactThreads = 256;
constexpr uint32_t kCompactItems = 8;                                   // consecutive entries per thread: 64 bytes, four 16-byte accesses
constexpr uint32_t kCompactSpan = kCompactThreads * kCompactItems;      // entries per block

struct CompactLevel {
    const SvoRecord* src;          // the old records: src_count in use
    const int32_t* src_leaves;     // the old leaf words: src_leaf_count in use
    SvoRecord* dst;                // the new records: dst_count entries
    int32_t* dst_leaves;           // the new leaf words: dst_leaf_count entries (the expand of the leaf parents' level only)
    uint64_t* part;                // per block of the level, then the total
    uint32_t src_count, src_leaf_count, dst_count, dst_leaf_count;
    uint32_t start, n;             // the level's entries of dst
    uint32_t leaf;                 // 1: the level of the leaf parents (the tree's depth)
};

// The blocks cover the entries from the even index at or below `start`, so that a thread's eight entries are 16-byte aligned.
inline uint32_t compact_blocks(uint32_t start, uint32_t n) { return uint32_t((uint64_t(start & 1u) + n + kCompactSpan - 1) / kCompactSpan); }

hipError_t launch_compact_count(const CompactLevel& a, hipStream_t s);
hipError_t launch_compact_expand(const CompactLevel& a, hipStream_t s);

}  // namespace vxrt
