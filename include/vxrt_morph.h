/*
 * vxrt_morph.h — morphology on a voxel list in device memory: dilate, erode, the surface layer and the margin ring, under the 6, 18
 * or 26 neighbourhood.  The optional extension of libvxrt.so for hosts that recolour the ring around a crater, keep only the hull
 * of a solid (the inside of a vxrt_voxelize_solid result or of a detached piece is never seen, and it is most of the voxels),
 * thicken a one-voxel mesh shell, close pinholes and drop specks after vxrt_transform_voxels_device or a carve, or put a collision
 * margin around a piece.  The list comes from vxrt_get_voxels_device, vxrt_detached_pieces_device, vxrt_transform_voxels_device,
 * vxrt_combine_voxels_device, a voxeliser or the host.  A host that only renders needs nothing from here.  Conventions as in
 * vxrt.h: 0 or a negative vxrt_status.
 *
 * The rule is exact and does not depend on schedule, device or call:
 *   1. the input S is the set of distinct positions of the list; the last entry of a position wins (vxrt_edit_voxels_device's
 *      rule, vxrt_transform.h's and vxrt_setops.h's rule 1) and its bytes are (mrgb[0] & 0x7f, r, g, b), as vxrt_get_voxels returns
 *      them: bit 7 of the material byte never matters
 *   2. the offset table has 26 rows: first the 6 offsets with one nonzero axis, then the 12 with two, then the 8 with three;
 *      within a class the rows ascend by 9 (dx + 1) + 3 (dy + 1) + (dz + 1).  Connectivity c (6, 18 or 26: vxrt_components.h's
 *      adjacency) uses the first c rows.  Coordinates do not wrap, and a neighbour outside the int16 range does not exist: it
 *      counts as empty
 *   3. one step of VXRT_MORPH_DILATE is S together with every cell of the range that has a neighbour in S.  A cell of S keeps its
 *      bytes; a new cell x takes the bytes of x + o_k for the least row k (of the first c) with x + o_k in S, so a face
 *      neighbour colours a new cell before an edge or corner neighbour does, at every connectivity.  One step of VXRT_MORPH_ERODE
 *      is the cells of S all of whose c neighbours are in S, with their own bytes; a cell on the edge of the int16 range always
 *      goes
 *   4. steps lies in 1 .. 64.  DILATE and ERODE apply their step `steps` times, each on the result of the one before, bytes
 *      included.  VXRT_MORPH_SURFACE is S without ERODE^steps(S), with S's bytes: the outer layer, `steps` cells thick.
 *      VXRT_MORPH_MARGIN is DILATE^steps(S) without S, with the bytes dilation gave: the ring outside
 *   5. the result is in ascending path order at depth 15, the order every device list of this library has (vxrt_extract.h); each
 *      position appears once
 *   6. values: the call carries bytes exactly when mrgb != NULL.  Then out_pos and out_mrgb come both or neither.  Without mrgb,
 *      out_mrgb must be NULL
 *   7. out_pos == out_mrgb == NULL counts only, and cap is ignored.  With arrays and more voxels than cap, *n_out is the count,
 *      nothing is written and the call returns VXRT_E_INVALID.  n == 0 gives *n_out = 0 without touching a device pointer
 *   8. every input byte is read before the first output byte is written (the input is copied into scratch keys first), so
 *      out_pos / out_mrgb may be the input's arrays
 *
 * Closing (dilate, then erode) and opening (erode, then dilate) are two calls.  The call needs no loaded scene and touches none.
 *
 * Ordering: the arrays are read and written on the context's stream, behind everything enqueued there; a producer on another stream
 * orders itself first with vxrt_context_wait_stream(ctx, producer_stream).  The call is synchronous: it waits for its own result, so
 * the arrays may be freed or rewritten when it returns; it does not call vxrt_sync.  Two calls with the same arguments write the
 * same bytes.
 *
 * Multi-GPU: call on each rank's context, in its own device's memory.
 */
#ifndef VXRT_MORPH_H
#define VXRT_MORPH_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vxrt_morph_op {
    VXRT_MORPH_DILATE  = 0,   /* S and every cell with a neighbour in S; a new cell takes its first source's bytes */
    VXRT_MORPH_ERODE   = 1,   /* the cells of S whose neighbours are all in S; their own bytes */
    VXRT_MORPH_SURFACE = 2,   /* S without ERODE^steps(S); S's bytes */
    VXRT_MORPH_MARGIN  = 3    /* DILATE^steps(S) without S; the bytes dilation gave */
} vxrt_morph_op;

/* pos[0 .. n), mrgb[0 .. n), out_pos[0 .. cap) and out_mrgb[0 .. cap) are device memory of the context's device and may have any
 * alignment; n_out is host memory.  op is a vxrt_morph_op, connectivity 6, 18 or 26, steps 1 .. 64.
 *
 * Scratch, freed before the call returns: about 24 bytes per entry of the list (vxrt_edit_voxels_device's front, run once); per
 * step 4 bytes per voxel of the current set and 12 per voxel of the step's result, and for a DILATE step about 36 bytes per offer
 * (an offer: a voxel of the set beside an empty cell of the range, at most c per voxel); 12 bytes per voxel of the result.  Every
 * allocation is made before the launches that use it, and the result's before the decode, the only kernel that writes an output
 * byte.
 *
 * Checked in this order:
 *   VXRT_E_INVALID  null context; n >= 2^32 (before any pointer is looked at); null n_out; op > 3; a connectivity that is not 6,
 *                   18 or 26; steps outside 1 .. 64; the values of rule 6; n > 0 with null pos
 *   n == 0          returns 0 with *n_out = 0 without touching a device pointer
 *   VXRT_E_INVALID  an array given that hipPointerGetAttributes does not report as device memory of the context's device, or that
 *                   ends past its allocation; the outputs at cap entries
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *   VXRT_E_INVALID  a step's offers or result number 2^32 or more
 *   VXRT_E_INVALID  arrays given and cap < the count (*n_out is the count)
 * A refused call writes nothing, and vxrt_last_error says why. */
int vxrt_morph_voxels_device(vxrt_ctx* ctx, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n,
                             uint32_t op, uint32_t connectivity, uint32_t steps,
                             int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_MORPH_H */
