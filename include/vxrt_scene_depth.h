/*
 * vxrt_scene_depth.h — the octree depth of a loaded scene changed in place: the optional extension of libvxrt.so for hosts that edit
 * (vxrt_edit.h, vxrt_grid_edit.h) past the root cube the scene was built with, or that want a scene emptied by clears to walk no more
 * levels than a fresh build of its voxels.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a
 * negative vxrt_status, all or nothing.
 *
 * Only the tree above the voxels changes: levels are added or removed on top of the root.  The voxels, their
 * coordinates, their order in vxrt_get_voxels and the temporal history stay; the sky cull's box stays (it still holds every voxel).
 * A call touches a few records per level changed; it reallocates the scene's storage (x 1.5) only when the storage has no room left,
 * as an edit does.  After a call every frame is bit-identical to the frame of a fresh context given the scene's voxel list by
 * vxrt_set_voxels whenever that list's depth rule gives the new depth — always after vxrt_fit_scene_depth.  Edits, grid edits, picks
 * and read-back work on the changed scene; at depth 15 an edit reaches every int16 position.
 *
 * Synchronous like vxrt_edit_voxels: frames enqueued before a call see the old scene.  Refusals, for both calls:
 *   VXRT_E_INVALID  null context; depth > 15; a scene with wide records or re-laid as treelets (as vxrt_edit_voxels)
 *   VXRT_E_NOSCENE  no scene set
 *   VXRT_E_SCENE    vxrt_set_scene_depth: shrinking would leave a voxel outside the new root cube.  vxrt_fit_scene_depth: the
 *                   scene is the one voxel (-32768, -32768, -32768), whose depth rule gives 16 (vxrt_set_voxels refuses that list)
 *   VXRT_E_DEVICE   the scene's storage could not grow (the old storage stays in place)
 *
 * Multi-GPU: every rank holds the whole scene, so a host makes the same call on every rank's context.
 */
#ifndef VXRT_SCENE_DEPTH_H
#define VXRT_SCENE_DEPTH_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Change the depth of the context's scene in place to `depth` (0..15): the root cube becomes [-2^depth, 2^depth)^3.  Growing is
 * always possible; shrinking only while every voxel lies in the smaller cube.  The current depth changes nothing. */
int vxrt_set_scene_depth(vxrt_ctx* ctx, uint32_t depth);

/* Set the depth that vxrt_set_voxels would give the scene's current voxel list; *depth (optional) receives it.  That is the least
 * depth whose root cube holds every voxel (0 for an empty scene), except for a scene that is the one voxel (-2^k, -2^k, -2^k): the
 * rule gives it k + 1 (src/context.rs's |max| + 1), so there the call grows the scene. */
int vxrt_fit_scene_depth(vxrt_ctx* ctx, uint32_t* depth);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_SCENE_DEPTH_H */
