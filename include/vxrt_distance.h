/*
 * vxrt_distance.h — the exact squared Euclidean distance transform of a voxel list in device memory, and what a threshold on it
 * gives: dilation and erosion by a ball.  The optional extension of libvxrt.so for hosts that fade a scorch mark with the true
 * distance from a crater's wall, ask how deep inside a wall or a detached piece a voxel lies before deciding what breaks, put a round
 * collision margin around a piece, close and open with a round element after vxrt_transform_voxels_device, or grow a crust of r cells
 * around a vxrt_voxelize_solid interior.  vxrt_morph.h steps one cell at a time under the 6, 18 or 26 neighbourhood and grows
 * diamonds and cubes; this call grows balls, in one pass whatever the radius.  The list comes from vxrt_get_voxels_device,
 * vxrt_detached_pieces_device, vxrt_transform_voxels_device, vxrt_combine_voxels_device, vxrt_morph_voxels_device, a voxeliser, a
 * rasteriser or the host.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status.
 *
 * The rule is exact and does not depend on schedule, device or call:
 *   1. the input S is the set of distinct positions of the list; the last entry of a position wins (vxrt_edit_voxels_device's rule,
 *      vxrt_transform.h's, vxrt_setops.h's and vxrt_morph.h's rule 1) and its bytes are (mrgb[0] & 0x7f, r, g, b), as vxrt_get_voxels
 *      returns them: bit 7 of the material byte never matters
 *   2. max_d2 lies in 1 .. 256 and is a SQUARED radius in cells.  R is the largest integer with R * R <= max_d2, at most 16.  A
 *      radius that is no integer is simply a max_d2 that is no square
 *   3. coordinates do not wrap.  A cell outside the int16 range holds no voxel, is never emitted, and counts as EMPTY for
 *      VXRT_DISTANCE_DEPTH and VXRT_DISTANCE_ERODE (vxrt_morph.h's rule 2): a voxel on the edge of the range has depth 1
 *   4. d2(a, b) = dx^2 + dy^2 + dz^2 in integers.  For a voxel v of S, depth(v) is the least d2(v, e) over the empty cells e with
 *      d2 <= max_d2, and VXRT_DISTANCE_FAR where there is none.  For an empty cell x of the range, field(x) is the least d2(x, s)
 *      over the s in S with d2 <= max_d2; a cell with none is not in the result
 *   5. with rank(0) = 0, rank(-k) = 2k - 1 and rank(+k) = 2k, the source of a FIELD cell x is the s in S that minimises
 *      (d2, rank(dz), rank(dy), rank(dx)) lexicographically, where (dx, dy, dz) = s - x.  The new cell takes the source's bytes.
 *      This is what a separable evaluation gives whose passes run along x, then y, then z and break ties by the rank of their own
 *      offset
 *   6. VXRT_DISTANCE_DEPTH: every voxel of S with depth(v) and its own bytes.  VXRT_DISTANCE_FIELD: every empty cell of the range
 *      that has a field value, with field(x) and its source's bytes.  VXRT_DISTANCE_ERODE: the voxels of S with depth(v) > max_d2
 *      (which is then VXRT_DISTANCE_FAR), with their own bytes: S eroded by the ball.  VXRT_DISTANCE_DILATE: S (d2 = 0, own bytes)
 *      together with FIELD's cells: S dilated by the ball
 *   7. the result is in ascending path order at depth 15, the order every device list of this library has (vxrt_extract.h); each
 *      position appears once
 *   8. values: the call carries bytes exactly when mrgb != NULL.  Then out_pos and out_mrgb come both or neither.  Without mrgb,
 *      out_mrgb must be NULL.  out_d2 is optional whenever out_pos is given, and must be NULL when out_pos is
 *   9. out_pos == NULL counts only, and cap is ignored.  With arrays and more voxels than cap, *n_out is the count, nothing is
 *      written and the call returns VXRT_E_INVALID.  n == 0 gives *n_out = 0 without touching a device pointer
 *  10. every input byte is read before the first output byte is written (the input is copied into scratch keys first), so the
 *      outputs may be the input's arrays
 *
 * Closing (DILATE, then ERODE of the result) and opening (ERODE, then DILATE) by a ball are two calls.  The call needs no loaded scene
 * and touches none.
 *
 * Ordering: the arrays are read and written on the context's stream, behind everything enqueued there; a producer on another stream
 * orders itself first with vxrt_context_wait_stream(ctx, producer_stream).  The call is synchronous: it waits for its own result, so
 * the arrays may be freed or rewritten when it returns; it does not call vxrt_sync.  Two calls with the same arguments write the
 * same bytes.
 *
 * Multi-GPU: call on each rank's context, in its own device's memory.
 */
#ifndef VXRT_DISTANCE_H
#define VXRT_DISTANCE_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vxrt_distance_mode {
    VXRT_DISTANCE_DEPTH  = 0,  /* every voxel of S: d2 to the nearest EMPTY cell, or FAR; S's bytes */
    VXRT_DISTANCE_FIELD  = 1,  /* every empty cell of the range with d2 to the nearest voxel of S <= max_d2; the source's bytes */
    VXRT_DISTANCE_ERODE  = 2,  /* the voxels of S whose DEPTH value is > max_d2 (FAR included); S's bytes */
    VXRT_DISTANCE_DILATE = 3   /* S (d2 = 0, own bytes) together with FIELD's cells */
} vxrt_distance_mode;
#define VXRT_DISTANCE_FAR    0xFFFFu
#define VXRT_DISTANCE_MAX_D2 256u

/* pos[0 .. n), mrgb[0 .. n), out_pos[0 .. cap), out_mrgb[0 .. cap) and out_d2[0 .. cap) are device memory of the context's device and
 * may have any alignment; n_out is host memory.  mode is a vxrt_distance_mode, max_d2 1 .. VXRT_DISTANCE_MAX_D2.
 *
 * Scratch, freed before the call returns: about 24 bytes per entry of the list (vxrt_edit_voxels_device's front, run once); 16
 * bytes per tile of S (a tile: an aligned cube of 16^3 cells that holds a voxel), and for FIELD and DILATE 27 times that and the
 * sort's digit counts.  Every allocation is made before the launches that use it.  The result goes straight into the caller's
 * arrays.
 *
 * Checked in this order:
 *   VXRT_E_INVALID  null context; n >= 2^32 (before any pointer is looked at); null n_out; mode > 3; max_d2 outside 1 .. 256; the
 *                   values of rule 8; n > 0 with null pos
 *   n == 0          returns 0 with *n_out = 0 without touching a device pointer
 *   VXRT_E_INVALID  an array given that hipPointerGetAttributes does not report as device memory of the context's device, or that
 *                   ends past its allocation; the outputs at cap entries (out_d2 at 2 * cap bytes)
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *   VXRT_E_INVALID  2^32 candidate tiles or result voxels or more
 *   VXRT_E_INVALID  arrays given and cap < the count (*n_out is the count)
 * A refused call writes nothing, and vxrt_last_error says why. */
int vxrt_distance_voxels_device(vxrt_ctx* ctx, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n,
                                uint32_t mode, uint32_t max_d2,
                                int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], uint16_t* out_d2, size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_DISTANCE_H */
