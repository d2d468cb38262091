/*
 * vxrt_extract.h — reading a loaded scene's voxels back from the device, whole or by box: the optional extension of libvxrt.so for
 * hosts that save what a user built (vxrt_edit.h) or inspect, copy or count a region of it.  A host that only renders needs nothing
 * from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status, host pointers borrowed for the call only.
 *
 * The voxels are decoded on the device from the records the tracers walk (DESIGN.md "Reading the scene back"), after any edits, on
 * every layout of the 8-byte records (breadth-first, with the holes and 8-entry blocks of edits, treelet order, beside the wide
 * records).  The list returned is one a fresh context can be given by vxrt_set_voxels: it builds the same octree, and every frame
 * renders bit-identically, as long as the depth is the same.
 *
 * Multi-GPU: every rank holds the whole scene, so any rank's context answers.
 */
#ifndef VXRT_EXTRACT_H
#define VXRT_EXTRACT_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The voxels of the context's scene, as it stands after everything enqueued so far, that lie in the half-open box
 * [box_min, box_max) (vxrt_set_voxels coordinates; both NULL = the whole root cube).  Waits for the result.
 *
 * Count first: with pos == mrgb == NULL the call only counts (cap is ignored): it sets *n and returns 0; nothing is materialised.
 * With buffers and cap < the count, it returns VXRT_E_INVALID, sets *n to the count and writes nothing.  Otherwise it writes the
 * *n voxels to pos[0 .. *n) and mrgb[0 .. *n).
 *
 * Order: ascending octree path.  With d the scene's depth (vxrt_stats.octree_depth) and u = p + 2^d per axis (0 <= u < 2^(d+1)),
 * the path of a voxel is the digits  s_k = (bit k of u.x) << 2 | (bit k of u.y) << 1 | (bit k of u.z)  for k = d, d-1, .., 0
 * (the root's first: the builder's child slot at every level), and the voxels come in ascending order of
 * key = sum over k of s_k << 3k.
 *
 * mrgb[i] = ((word >> 24) & 0x7f, r, g, b) of the voxel's leaf word: what vxrt_set_voxels turns back into the same word.
 *
 * Boxes are int32, so a box may reach past the int16 range; only its part inside the root cube [-2^d, 2^d)^3 counts.  A box that is
 * empty on some axis (box_min >= box_max) or lies outside the root cube gives *n = 0 and VXRT_OK.
 *
 *   VXRT_E_INVALID  null context, null n, exactly one of box_min / box_max NULL, exactly one of pos / mrgb NULL, cap < the count
 *   VXRT_E_NOSCENE  no scene set
 *   VXRT_E_DEVICE   the decode's scratch could not be allocated (nothing is written)
 *
 * The call changes no scene byte, no image and no temporal history: frames enqueued before or after it render as they would
 * without it.  The scratch it uses (the decode's frontier, scan partials and output staging) belongs to the context, grows as
 * needed and is freed by vxrt_destroy. */
int vxrt_get_voxels(vxrt_ctx* ctx, const int32_t box_min[3], const int32_t box_max[3], int16_t (*pos)[3], uint8_t (*mrgb)[4],
                    size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_EXTRACT_H */
