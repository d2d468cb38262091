/*
 * vxrt_device_scene.h — building a scene on the device from a voxel list that already lives in device memory: the optional extension
 * of libvxrt.so for hosts whose voxels come from the GPU (a torch pipeline, a voxeliser, a simulation, vxrt_get_voxels of another
 * context) or whose lists are too large for the host builder.  A host that only renders needs nothing from here.  Conventions as in
 * vxrt.h: 0 or a negative vxrt_status.
 *
 * The octree is built by device kernels: a stable radix sort of the voxels' path keys, a dedupe, then the node
 * levels bottom-up from prefix sums.  Every position is a prefix sum in input order, so two calls on the same list write the same
 * bytes.
 *
 * Multi-GPU: every rank holds the whole scene; give each rank's context the list in its own device's memory.
 */
#ifndef VXRT_DEVICE_SCENE_H
#define VXRT_DEVICE_SCENE_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* vxrt_set_voxels with pos[0 .. n) and mrgb[0 .. n) in device memory of the context's device (hipMalloc, or a torch tensor's
 * storage).  The result is what vxrt_set_voxels of the same list does to the context: the same 8-byte records and leaf words, byte
 * for byte (the last entry for a position wins; the depth follows the same rule), the same depth, sky-cull box and vxrt_stats, the
 * same VXRT_OPT_NODE_ORDER and VXRT_OPT_SCENE_FORMAT handling, and the temporal history is reset as a new scene resets it.
 *
 * Ordering: the call reads the arrays on the context's stream, behind everything enqueued there.  A producer on another stream
 * orders itself first with vxrt_context_wait_stream(ctx, producer_stream).  The call is synchronous: it returns when the scene is
 * set, and the arrays may be freed or rewritten from then on.
 *
 * Size: unlike the host builder, which refuses trees of 2^26 nodes or more, this one builds any tree whose records and leaf words
 * fit the 32-bit base field.  Its scratch, freed before it returns, is about 24 bytes per voxel.
 *
 *   VXRT_E_INVALID  null context; n > 0 with a null array; n >= 2^32; an array that hipPointerGetAttributes does not report as
 *                   device memory of the context's device (pageable, pinned or managed host memory included), or that ends past
 *                   its allocation
 *   VXRT_E_SCENE    depth > 15, or 2^32 records or more
 *   VXRT_E_DEVICE   the scratch or the new scene could not be allocated
 *
 * A refused call changes nothing: the previous scene stays, byte for byte, and renders as before. */
int vxrt_set_voxels_device(vxrt_ctx* ctx, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_DEVICE_SCENE_H */
