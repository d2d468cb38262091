// edit.h — what api_edit.hip (host side of vxrt_edit.h) and edit.hip (its kernels) share, and what the device-side editors
// (grid_edit.hip, api_device_edit.hip / device_edit.hip) add in front of the same tail.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/vxrt_edit.h"
#include "kernels.h"
#include "owned.h"

namespace vxrt {

using ScratchBuffer = DeviceBuf<void>;   // ctx.h

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
// and gives the device arrays and the kernel's scratch (node, flag: seg_off[depth + 1] entries each; out: 8 words) itself, and so
// does vxrt_edit_voxels_device (cut_edit_lists below).
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

// The cut, on the device (grid_edit.hip), of `count` (1 or 2) lists of path keys at depth L, each ascending and unique (m[b] < 2^32
// entries, none when 0), into edit_kernel's segments.  For every non-empty list, *out[b] gets seg_off, child_begin, oct and the
// kernel's scratch (node, flag, out: one set, shared by the lists, which are applied one after the other); clear, words, lo and hi
// stay the caller's to fill.  Every device array lives in *batch.  Runs on `stream` and waits.  VXRT_E_DEVICE: an allocation failed.
int cut_edit_lists(const uint64_t* const* keys, const uint32_t* m, int count, uint32_t L, hipStream_t stream, const char* who,
                   ScratchBuffer* batch, EditBatch* const* out);

// One pass over a device voxel list at the scene's depth (device_edit.hip): keys[i] = entry i's path key, vals[i] = its leaf word
// (mrgb and vals null: a clear), and the list's least and greatest position per axis and whether any lies outside the root cube
// [-2^depth, 2^depth)^3, reduced on the device and read back once.  n > 0.  Waits.  VXRT_E_DEVICE: an allocation failed.
struct ListBounds {
    int32_t lo[3], hi[3];
    uint32_t outside, pad;
};
int edit_keys_device(const int16_t* pos, const uint8_t* mrgb, size_t n, uint32_t depth, uint64_t* keys, uint32_t* vals, hipStream_t stream,
                     const char* who, ListBounds* out);

// The storage for `svo_need` records and `leaf_need` leaf words: fresh arrays (at the capacities svo_cap / leaf_cap, holding the
// arrays in use and zeros after them) where the current ones are too small (x 1.5), empty where they are not.
// Nothing changes in the context; a failure, or a GrownStorage that is never committed, leaves nothing allocated.
// VXRT_E_SCENE: 2^32 records or leaf words.
struct GrownStorage {
    DeviceBuf<SvoRecord> svo;
    DeviceBuf<int32_t> leaves;
    size_t svo_cap = 0, leaf_cap = 0;
};
int grow_storage(vxrt_ctx* c, size_t svo_need, size_t leaf_need, GrownStorage* g);
// ... and the grown storage replaces the old
void commit_storage(vxrt_ctx* c, GrownStorage&& g);

// Room for a set batch with `nodes` segments on node levels 0 .. depth - 1 and `parents` leaf parents: the storage grows
// (geometrically) when it has to.  VXRT_E_SCENE: 2^32 records or leaf words; VXRT_E_DEVICE: the storage could not grow (nothing
// changed).  Call after sync_all.
int reserve_edit_storage(vxrt_ctx* c, size_t nodes, size_t parents);

// The tail of an edit, shared by vxrt_edit_voxels, vxrt_edit_voxel_grid and vxrt_edit_voxels_device: storage growth, the `edited` bookkeeping, the launch, the
// counters, the touch maps and the sky cull's box.  Drains the frames in flight first; waits for the edit.  All or nothing.
int apply_edit_batch(vxrt_ctx* c, const EditBatch& b);

// vxrt_scene_depth.h (scene_depth.hip; api_scene_depth.hip): one wave each, lane o < 8 takes octant o of the root (record `root`,
// d_svo[0], at depth `depth`, child mask non-zero).
//   probe   out[0] = the levels the scene can lose: the least, over the root's children o, of the levels 1, 2, ... whose node on o's
//           path has slot o ^ 7 only; out[1] = 1 when the scene is the one voxel (-2^t, -2^t, -2^t) of depth t = depth - out[0]
//   grow    `levels` levels on top: the root keeps its mask and gets an 8-entry block at svo_end; its child o becomes a chain of
//           `levels` nodes with slot o ^ 7 only, each with an 8-entry block of its own (records from svo_end + 8, chain by chain,
//           in octant order; with depth 0 the chain's last block is 8 leaf words from leaf_end), the last holding the old child o
//   shrink  `levels` levels off the top (the probe allowed it): slot o of the root's block takes the record `levels` levels below it
//           on o's path; with levels == depth the root becomes a leaf parent of an 8-entry leaf block at leaf_end
hipError_t launch_depth_probe(const SvoRecord* svo, SvoRecord root, uint32_t depth, uint32_t* out, hipStream_t s);
hipError_t launch_depth_grow(SvoRecord* svo, int32_t* leaves, SvoRecord root, uint32_t depth, uint32_t levels, uint32_t svo_end,
                             uint32_t leaf_end, hipStream_t s);
hipError_t launch_depth_shrink(SvoRecord* svo, int32_t* leaves, SvoRecord root, uint32_t depth, uint32_t levels, uint32_t leaf_end,
                               hipStream_t s);

}  // namespace vxrt
