// query.h — what api_query.hip (host side of vxrt_query.h) and query.hip (its kernels) share.  DESIGN.md §22.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ctx.h"
#include "../../include/vxrt_edit.h"

namespace vxrt {

// The lookup runs blocks of kQueryThreads threads over kQuerySpan consecutive entries each, kQueryItems entries per thread (the
// layout of extract.hip and components.hip), so a grid has query_blocks(n) <= 2^21 blocks for n < 2^32.
constexpr uint32_t kQueryThreads = 256;
constexpr uint32_t kQueryItems = 8;
constexpr uint32_t kQuerySpan = kQueryThreads * kQueryItems;
constexpr uint32_t kQueryLevels = 16;   // node levels 0 .. depth of the deepest tree int16 positions allow (depth 15)

inline uint32_t query_blocks(uint64_t n) { return uint32_t((n + kQuerySpan - 1) / kQuerySpan); }

struct LookupArgs {
    const SvoRecord* svo;
    const int32_t* leaves;
    SvoRecord root_rec;     // svo[0]: every descent begins with it
    uint32_t depth;         // the leaf parents' node level, <= 15
    int32_t offset[3];
    const int16_t* pos;     // n entries, any alignment
    uint32_t n;
    uint32_t* leaf;         // n words, or nullptr
    uint64_t* part;         // query_blocks(n) counts, or nullptr
};

// leaf[i] = the leaf word at pos[i] + offset or 0 (vxrt_query.h's rule); part[b] = the nonzero answers among block b's entries.
hipError_t launch_query_lookup(const LookupArgs& a, hipStream_t s);

// The pick's view of the loaded scene: the 8-byte records only, whatever format the tracers walk.
inline TraceArgs pick_args(const vxrt_ctx* c) {
    TraceArgs a{};
    a.svo = c->d_svo;
    a.leaves = c->d_leaves;
    a.root_rec = c->root_rec;
    a.node_levels = int(c->depth) + 1;
    memcpy(a.root_center, c->root_center, sizeof a.root_center);
    a.root_size = c->root_size;
    a.stack_levels = c->depth < 1 ? 1 : int(c->depth);
    return a;
}

// The pick of vxrt_pick and vxrt_pick_device: cast_ray per ray, bounded by max_time[i] (nullptr: every ray unbounded), n > 0 rays in
// blocks of kBlock.  a: pick_args.
hipError_t launch_query_pick(const TraceArgs& a, const float* origins, const float* dirs, const float* max_time, vxrt_pick_hit* out,
                             unsigned n, hipStream_t s);

}  // namespace vxrt
