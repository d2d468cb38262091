/*
 * vxrt_compact.h — an edited scene's octree put back into the bytes of a fresh build, in place on the device: the optional extension
 * of libvxrt.so for hosts that edit a loaded scene for a long time (vxrt_edit.h, vxrt_grid_edit.h, vxrt_device_edit.h,
 * vxrt_scene_depth.h).  A host that only renders, or edits a little, needs nothing from here.  Conventions as in vxrt.h: 0 or a
 * negative vxrt_status, all or nothing.
 *
 * Edits never give storage back: a node that comes into being gets an 8-entry block after the end of the arrays, and the block of a
 * node that is pruned or moves stays behind as a hole.  A region that is cleared and set again therefore grows
 * the arrays with every cycle, up to the 2^32-entry limit at which edits are refused.  vxrt_get_scene_storage says how much of the
 * storage is holes; vxrt_compact_scene removes them.
 *
 * vxrt_compact_scene keeps the tree — the depth, every mask, every leaf word, the order of vxrt_get_voxels, every pick and every
 * frame — and gives it the layout of a fresh build: records breadth first and level by level, every block tight, the leaf words in
 * the order of their parents, both arrays allocated at exactly the live sizes.  When the scene's depth is what vxrt_set_voxels would
 * give its voxel list (always after vxrt_fit_scene_depth), the device holds byte for byte what a fresh context given that list holds.
 * The sky cull's box is recomputed from the new records, so it can shrink to a fresh build's; the temporal history stays.  The next
 * edit starts the storage rule over from the compacted counts.
 *
 * Synchronous like vxrt_edit_voxels: frames enqueued before the call see the old arrays.  The new arrays are written beside the old
 * ones and swapped in at the end; while it runs the call needs the live sizes on top of the storage in place.  Refusals:
 *   VXRT_E_INVALID  null context or null `out`; vxrt_compact_scene: a scene with wide records or re-laid as treelets (as vxrt_edit_voxels)
 *   VXRT_E_NOSCENE  no scene set
 *   VXRT_E_DEVICE   vxrt_compact_scene: the new arrays could not be allocated (the old storage stays in place)
 *   VXRT_E_SCENE    vxrt_compact_scene: the records reached from the root are not as many as the context counts (nothing changes)
 *
 * Multi-GPU: every rank holds the whole scene, so a host makes the same call on every rank's context.
 */
#ifndef VXRT_COMPACT_H
#define VXRT_COMPACT_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Re-lay the context's scene as a fresh build of the same tree would lie, on the device.  A scene that was never edited is left as
 * it is. */
int vxrt_compact_scene(vxrt_ctx* ctx);

/* The scene's storage as the context counts it (no device work).  Holes are records_used - records_live; after a build or a
 * compaction records_live == records_used == records_capacity and leaves_used == leaves_capacity. */
typedef struct vxrt_scene_storage {
    uint64_t records_live, records_used, records_capacity;   /* 8-byte records: in the tree / up to the end in use / allocated */
    uint64_t leaves_used, leaves_capacity;                    /* leaf words: up to the end in use / allocated                  */
} vxrt_scene_storage;
int vxrt_get_scene_storage(vxrt_ctx* ctx, vxrt_scene_storage* out);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_COMPACT_H */
