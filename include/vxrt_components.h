/*
 * vxrt_components.h — the connected components of a voxel list in device memory, and the voxels of the loaded scene that are no
 * longer attached to anything: the optional extension of libvxrt.so for hosts that break things.  After a voxel is broken under the
 * cursor (vxrt_edit.h), a shape is carved out (vxrt_solid.h) or a simulation step cleared its debris (vxrt_device_edit.h), the
 * question is which voxels now hang in the air.  vxrt_detached_voxels_device answers it on the device, as a list that
 * vxrt_edit_voxels_device clears and the host re-emits as debris; vxrt_label_components_device is the labelling under it, for any
 * list.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status.
 *
 * The rule is exact and does not depend on schedule, device or call:
 *   1. two entries are adjacent when their positions are equal, or differ by at most 1 on every axis and on at most 1, 2 or 3 axes:
 *      connectivity 6 (faces), 18 (faces and edges), 26 (faces, edges and corners)
 *   2. coordinates do not wrap: 32767 and -32768 are not neighbours
 *   3. a component is a class of the transitive closure of adjacency
 *   4. label[i] is the least index j in [0, n) of an entry in i's component
 *   5. the number of components is the number of i with label[i] == i
 * For a list in path order (vxrt_get_voxels_device, vxrt_device_edit.h) a label is therefore the index of its component's first voxel
 * in path order.
 *
 * Multi-GPU: every rank holds the whole scene; label on each rank's context, in its own device's memory.
 */
#ifndef VXRT_COMPONENTS_H
#define VXRT_COMPONENTS_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pos[0 .. n) and label[0 .. n) are device memory of the context's device; label is 4-byte aligned, pos may have any alignment.  The
 * list may be in any order and may hold a position more than once.  connectivity is 6, 18 or 26.  label == NULL counts only; n == 0
 * gives *n_components == 0 without touching a pointer.  No scene is needed and none is touched; pos is never written.
 *
 * Ordering: the list is read on the context's stream, behind everything enqueued there; a producer on another stream orders itself
 * first with vxrt_context_wait_stream(ctx, producer_stream).  The call is synchronous: it returns when label is written, and the
 * arrays may be freed or rewritten from then on.  Two calls on the same list write the same bytes.
 *
 * Scratch, freed before the call returns: about 40 bytes per entry.  Every scratch allocation happens before a byte of label is
 * written.
 *
 *   VXRT_E_INVALID  null context or n_components; n > 0 with null pos; n >= 2^32 (checked before any pointer is looked at); a
 *                   connectivity other than 6, 18 or 26; an array that hipPointerGetAttributes does not report as device memory of
 *                   the context's device, or that ends past its allocation; a misaligned label
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *
 * A refused call writes nothing. */
int vxrt_label_components_device(vxrt_ctx* ctx, const int16_t (*pos)[3], size_t n, uint32_t connectivity, uint32_t* label,
                                 size_t* n_components);

/* The voxels of the loaded scene, as it stands, whose component holds no voxel inside the half-open anchor box
 * [anchor_min, anchor_max): what no longer hangs on the ground, a wall, or whatever the box covers.  Components are taken over the
 * whole scene, by the rule above.  The result is in ascending path order, with the bytes vxrt_get_voxels (vxrt_extract.h) returns;
 * pos, mrgb, cap and n are vxrt_get_voxels_device's (vxrt_device_edit.h), with the same pointer checks, count-only form
 * (pos == mrgb == NULL) and cap rule: with more detached voxels than cap, *n is the count, nothing is written and the call returns
 * VXRT_E_INVALID.  An anchor box that is empty or misses the scene returns every voxel; a scene with no voxel gives *n == 0.  The
 * call reads scenes in any record order and format, as the extract does, runs on the context's stream and waits for the result.  It
 * changes no scene byte, image or history.  vxrt_edit_voxels_device(ctx, pos, NULL, *n) clears the returned list.
 *
 * Scratch, freed before the call returns: about 54 bytes per voxel of the scene, all of it allocated before an output byte is
 * written.
 *
 *   VXRT_E_INVALID  null context, n or anchor pointer; a connectivity other than 6, 18 or 26; everything vxrt_get_voxels_device
 *                   refuses as invalid
 *   VXRT_E_NOSCENE  no scene is loaded
 *   VXRT_E_DEVICE   the scratch could not be allocated */
int vxrt_detached_voxels_device(vxrt_ctx* ctx, const int32_t anchor_min[3], const int32_t anchor_max[3], uint32_t connectivity,
                                int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_COMPONENTS_H */
