// edit.h — what api_edit.hip (host side of vxrt_edit.h) and edit.hip (its kernels) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vxrt_edit.h"
#include "kernels.h"

namespace vxrt {

// A batch as edit_kernel walks it: the entries, sorted by octree path and one per position, cut into "segments" per tree level —
// segment = one node on the path of at least one entry.  Node levels run 0 (the root: one segment) .. depth (the leaf parents);
// the segments of level depth + 1 are the entries themselves.  All segments are numbered level by level (seg_off[l] .. seg_off[l+1]
// are level l's), each in path order, so the children of segment s are the segments child_begin[s] .. child_begin[s + 1] - 1 of the
// next level and oct[c] is the slot segment c takes in its parent.
struct EditArgs {
    SvoRecord* svo;
    int32_t* leaves;
    const uint32_t* child_begin;  // segments of levels 0 .. depth, + 1
    const uint8_t* oct;           // every segment (the root's is 0)
    const int32_t* words;         // sets: the leaf word of every entry (level depth + 1, in segment order)
    uint32_t* node;               // scratch: the record of every segment of levels 0 .. depth
    uint8_t* flag;                // scratch (clears): the segment's node lost its last entry
    uint32_t* out;                // [0] records in use, [1] leaf words in use, [2] records added (sets) / removed (clears), [3..4] the root
    uint32_t seg_off[18];         // depth <= 15 (scene_host.cpp: build_octree): levels 0 .. 16 and the end
    uint32_t depth;
    uint32_t svo_end, leaf_end;        // records / leaf words in use: new 8-entry blocks start here
    uint32_t svo_built, leaf_built;    // ... as the scene was built: a block below these is tight, one at or above holds 8 entries
    int clear;
};

hipError_t launch_edit(const EditArgs& a, hipStream_t s);

// A batch cut into segments, as the tail of an edit takes it (api_edit.hip: apply_edit_batch).  vxrt_edit_voxels cuts on the host
// and hands the arrays over in `host` (child_begin | words | oct, uploaded in one copy); vxrt_edit_voxel_grid cuts on the device
// and gives the device arrays and the kernel's scratch (node, flag: seg_off[depth + 1] entries each; out: 8 words) itself.
struct EditBatch {
    uint32_t seg_off[18];                       // as EditArgs, levels 0 .. depth + 1 and the end
    bool clear = false;
    int32_t lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};   // sets: the least and greatest set position per axis (the sky cull's box grows by them)
    const uint8_t* host = nullptr;              // host arrays: `host_bytes` bytes, words at host_words, oct at host_oct
    size_t host_bytes = 0, host_words = 0, host_oct = 0;
    const uint32_t* child_begin = nullptr;      // device arrays (host == nullptr)
    const uint8_t* oct = nullptr;
    const int32_t* words = nullptr;
    uint32_t* node = nullptr;
    uint8_t* flag = nullptr;
    uint32_t* out = nullptr;
};

// Room for a set batch with `nodes` segments on node levels 0 .. depth - 1 and `parents` leaf parents: the storage grows
// (geometrically) when it has to.  VXRT_E_SCENE: 2^32 records or leaf words; VXRT_E_DEVICE: the storage could not grow (nothing
// changed).  Call after sync_all.
int reserve_edit_storage(vxrt_ctx* c, size_t nodes, size_t parents);

// The tail of an edit, shared by vxrt_edit_voxels and vxrt_edit_voxel_grid: storage growth, the `edited` bookkeeping, the launch, the
// counters, the touch maps and the sky cull's box.  Drains the frames in flight first; waits for the edit.  All or nothing.
int apply_edit_batch(vxrt_ctx* c, const EditBatch& b);
hipError_t launch_pick(const TraceArgs& a, const float* origins, const float* dirs, vxrt_pick_hit* out, unsigned n, hipStream_t s);

}  // namespace vxrt
