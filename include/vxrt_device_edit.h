/*
 * vxrt_device_edit.h — editing and reading a loaded scene through voxel lists that live in device memory: the optional extension of
 * libvxrt.so for hosts whose sparse edits are produced on the GPU (debris or particles of a simulation step, a voxeliser's output, a
 * brush evaluated in torch, nonzero of a mask) and for pipelines that read a box, transform it on the device and write it back.  A
 * host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status.
 *
 * The list is keyed at the scene's depth, sorted, deduplicated and cut into the edit kernel's segments by device kernels
 * (DESIGN.md §15); nothing but a few counters crosses to the host.  Every position is a prefix sum in input order, so two calls on
 * the same list write the same bytes.
 *
 * Multi-GPU: every rank holds the whole scene; give each rank's context the list in its own device's memory.
 */
#ifndef VXRT_DEVICE_EDIT_H
#define VXRT_DEVICE_EDIT_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vxrt_edit_voxels (vxrt_edit.h) with pos[0 .. n) and mrgb[0 .. n) in device memory of the context's device (hipMalloc, or a torch
 * tensor's storage).  mrgb == NULL clears the listed positions (absent ones are ignored); otherwise they are set, and the last entry
 * for a position wins.  After the call the context is, byte for byte, what vxrt_edit_voxels of the same list leaves: the records and
 * leaf words in use, the storage (grown x 1.5, new nodes in 8-entry blocks), vxrt_stats, the sky-cull box (grown by the least and
 * greatest listed position per axis), the kept temporal history and every later frame.  n == 0 does nothing.
 *
 * Ordering: frames enqueued before the call see the old scene.  The call reads the arrays on the context's stream, behind
 * everything enqueued there; a producer on another stream orders itself first with vxrt_context_wait_stream(ctx, producer_stream).
 * The call is synchronous: it returns when the scene is edited, and the arrays may be freed or rewritten from then on.
 *
 * Scratch, freed before the call returns: about 24 bytes per entry (16 for a clear) plus the segment arrays.  Every scratch
 * allocation and the storage reservation happen before a scene byte changes.
 *
 *   VXRT_E_INVALID  null context; n > 0 with null pos; n >= 2^32; an array that hipPointerGetAttributes does not report as device
 *                   memory of the context's device (pageable, pinned or managed host memory included), or that ends past its
 *                   allocation; a scene in wide records (VXRT_OPT_SCENE_FORMAT 1) or in treelet order (VXRT_OPT_NODE_ORDER 2 / 3)
 *   VXRT_E_NOSCENE  no scene is loaded
 *   VXRT_E_SCENE    a position outside the scene's root cube [-2^depth, 2^depth)^3 (vxrt_last_error gives the list's bounds and
 *                   the cube), or a scene that would reach 2^32 records or leaf words
 *   VXRT_E_DEVICE   the scratch or the grown storage could not be allocated
 *
 * A refused call changes nothing: the scene stays, byte for byte, and renders as before. */
int vxrt_edit_voxels_device(vxrt_ctx* ctx, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n);

/* vxrt_get_voxels (vxrt_extract.h) with pos and mrgb in device memory of the context's device: the voxels of the scene as it stands
 * in the half-open box [box_min, box_max) (both NULL: the whole root cube), in ascending path order, the same count, positions and
 * bytes.  pos == mrgb == NULL counts only.  With arrays, cap is their room in voxels: when the box holds more, *n is the count,
 * nothing is written and the call returns VXRT_E_INVALID.  The decode runs on the context's stream, behind everything enqueued
 * there, and writes into the caller's arrays; nothing crosses to the host but *n.  The call waits for the result.  It changes no
 * scene byte, image or history, and reads scenes in any record order and format, as vxrt_get_voxels does.
 *
 *   VXRT_E_INVALID  null context or n; one of box_min / box_max or of pos / mrgb without the other; arrays that are not device
 *                   memory of the context's device or that end before cap voxels; cap < the count
 *   VXRT_E_NOSCENE  no scene is loaded
 *   VXRT_E_DEVICE   the scratch could not be allocated */
int vxrt_get_voxels_device(vxrt_ctx* ctx, const int32_t box_min[3], const int32_t box_max[3], int16_t (*pos)[3], uint8_t (*mrgb)[4],
                           size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_DEVICE_EDIT_H */
