/*
 * vxrt_edit.h — editing a loaded scene in place, and picking the voxel a ray hits: the optional extension of libvxrt.so for hosts
 * that edit (an interactive renderer that places, breaks or recolours voxels under the cursor).  A host that only renders needs
 * nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status, host pointers borrowed for the call only.
 *
 * The scene is edited on the device, in the records the tracers walk (DESIGN.md "Scene edits"): no octree is rebuilt, nothing
 * is uploaded but the edits, the temporal history is kept, and the device-built procedural scene (vxrt_set_menger) can be edited
 * like any other.  After any sequence of edits every frame is bit-identical to the frame of a fresh context given the edited
 * voxel list by vxrt_set_voxels, as long as that list has the same octree depth: an edit never changes the depth.
 *
 * Multi-GPU: every rank holds the whole scene, so a host applies the same edits, in the same order, on every rank's context.
 */
#ifndef VXRT_EDIT_H
#define VXRT_EDIT_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Set (mrgb != NULL: insert or overwrite) or clear (mrgb == NULL: remove; absent positions are ignored) n voxels of the
 * context's scene in place.  Positions and leaf words follow vxrt_set_voxels (material & 0x7f, r, g, b); within one call the
 * last entry for a position wins.  Synchronous like vxrt_set_voxels: frames enqueued before the call see the old scene, frames
 * after it the new one; the temporal history is kept (temporal.comp's depth and normal test decides what survives an edit;
 * vxrt_reset_history makes a hard cut).
 * All or nothing — a refused call changes nothing:
 *   VXRT_E_INVALID  null context, null pos with n > 0, a scene with wide records (VXRT_OPT_SCENE_FORMAT 1) or re-laid as treelets
 *                   (VXRT_OPT_NODE_ORDER 2 / 3)
 *   VXRT_E_NOSCENE  no scene set
 *   VXRT_E_SCENE    a position outside the root cube [-2^d, 2^d)^3 of the scene's depth d (vxrt_stats.octree_depth)
 *   VXRT_E_DEVICE   the scene's storage could not grow (the old storage stays in place)
 * n == 0 does nothing. */
int vxrt_edit_voxels(vxrt_ctx* ctx, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n);

typedef struct vxrt_pick_hit {
    uint32_t status;     /* 0 miss, 1 hit, 2 the walk reached its 2048-trip cap (voxels.comp:166-169): no voxel              */
    float time;          /* as cast_bounded_ray returns it                                                                    */
    float normal[3];     /* the hit face's outward normal (0 on a miss or at the cap)                                          */
    int32_t voxel[3];    /* status 1: the voxel the walk stopped in, in vxrt_set_voxels coordinates; 0 otherwise              */
    int32_t leaf;        /* status 1: its leaf word (0x80000000 | material << 24 | rgb); 2: 0x80000000; 0: 0                    */
} vxrt_pick_hit;

/* Cast n rays (origins, directions in world units, as the tracers cast them) against the scene as it stands after everything
 * enqueued so far; waits for the result.  status, time, normal and leaf are those of the tracers' own walk, bit for bit.
 * A non-finite origin means what the shader's root test makes of it by compare and select, x first: an infinite
 * coordinate or a NaN in origin[0] is a miss with time 0; a NaN in origin[1] or [2] alone is dropped and the ray stays on that axis' low side.
 * A time of zero may come back as -0 where the shader's is +0 (an origin exactly on a voxel plane); nothing else ever differs. */
int vxrt_pick(vxrt_ctx* ctx, const float (*origins)[3], const float (*dirs)[3], size_t n, vxrt_pick_hit* out);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_EDIT_H */
