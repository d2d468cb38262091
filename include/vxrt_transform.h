/*
 * vxrt_transform.h — a voxel list in device memory resampled under an affine map given in fixed point: the optional extension of
 * libvxrt.so for hosts that turn, mirror, scale or re-sample what they hold as a list.  A loose piece (vxrt_pieces.h) that became a
 * rigid body turns as well as moves; a stamp or prefab is placed rotated or mirrored; debris is shown at half resolution.  The list
 * comes from vxrt_detached_pieces_device, vxrt_get_voxels_device, a voxeliser (vxrt_voxelize.h, vxrt_solid.h) or the host, and the
 * result goes to vxrt_lookup_voxels_device (the collision test), vxrt_edit_voxels_device or vxrt_set_voxels_device, without a round
 * trip through the host.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status.
 *
 * The map is applied by pulling: every cell of a destination box asks the source list which voxel its centre comes from, so the
 * result has no holes, no duplicates and one answer per cell.  The rule is exact and does not depend on schedule, device or call
 * (DESIGN.md §23):
 *   1. the source is the set of distinct positions of pos[0 .. n); the last entry of a position wins (vxrt_edit_voxels_device's
 *      rule) and its bytes are (mrgb[0] & 0x7f, r, g, b), as vxrt_get_voxels returns them
 *   2. for a destination cell d of the half-open box [box_min, box_max), per axis i:  P_i = sum_j m[i][j] * (2 d_j + 1) + 2 t[i]  in
 *      64 bits (the limits below keep |P_i| under 2^43, so no sum wraps), and the source cell is  s_i = P_i >> 17,  an arithmetic
 *      shift: the floor of  M (d + 1/2) + t,  the cell that holds the pulled centre
 *   3. d is in the result exactly when all three s_i lie in [-32768, 32767] and s is a source position; the range test is made on
 *      the 64-bit values before anything is narrowed, so a pulled centre outside the int16 range is absent, never wrapped; the voxel
 *      at d carries the bytes of s
 *   4. the result is written in ascending path order, the order every device list of this library has (vxrt_extract.h); that order
 *      does not depend on a depth
 *   5. mrgb == NULL means positions only, and out_mrgb must then be NULL too; out_pos == out_mrgb == NULL counts only, and cap is
 *      ignored; with arrays and more voxels than cap, *n_out is the count, nothing is written and the call returns VXRT_E_INVALID
 *   6. an empty box (box_min[i] >= box_max[i] on any axis) or n == 0 gives *n_out = 0 without touching a device pointer
 *
 * A rigid pull map.  Points of a body move by  x -> R (x - p) + p + u  (R a rotation, p a pivot, u a translation) in the coordinates
 * in which cell c is the cube [c, c + 1)^3; p may be a half-integer, and a piece's centre of mass is vxrt_piece's sum / voxels + 1/2
 * per axis.  The pull is the inverse:
 *      m[i][j] = rint(65536 * R[j][i])                                  (the transpose)
 *      t[i]    = rint(65536 * (p_i - sum_j R[j][i] * (p_j + u_j)))
 * in double precision with rint() of <math.h>.  The destination box is the forward image of the source's cell box, grown by 2 cells
 * per side (the rounding of m moves a pulled centre by less than half a cell within the int16 range) and clipped to
 * [-32768, 32768].  The 24 axis rotations and the mirrors have m in {0, +-65536} and are exact bijections of the cells.
 *
 * The call needs no loaded scene, touches none, and never writes pos or mrgb.
 *
 * Ordering: the arrays are read and written on the context's stream, behind everything enqueued there; a producer on another stream
 * orders itself first with vxrt_context_wait_stream(ctx, producer_stream).  The call is synchronous: it waits for its own result, so
 * the arrays may be freed or rewritten when it returns.  Two calls with the same arguments write the same bytes.
 *
 * Multi-GPU: call on each rank's context, in its own device's memory.
 */
#ifndef VXRT_TRANSFORM_H
#define VXRT_TRANSFORM_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vxrt_affine {
    int32_t m[3][3];    /* Q16: 65536 is 1.0; |m[i][j]| <= 2^24 */
    int32_t reserved;   /* must be 0 */
    int64_t t[3];       /* Q16, in cells; |t[i]| <= 2^40 */
} vxrt_affine;          /* 64 bytes, 8-byte aligned; host memory */

#ifdef __cplusplus
static_assert(sizeof(vxrt_affine) == 64 && alignof(vxrt_affine) == 8, "vxrt_affine");
#else
typedef char vxrt_affine_is_64_bytes[sizeof(vxrt_affine) == 64 ? 1 : -1];
typedef char vxrt_affine_is_8_byte_aligned[(sizeof(struct { char c; vxrt_affine a; }) - sizeof(vxrt_affine)) == 8 ? 1 : -1];
#endif

/* pos[0 .. n), mrgb[0 .. n), out_pos[0 .. cap) and out_mrgb[0 .. cap) are device memory of the context's device and may have any
 * alignment; pull, box_min, box_max and n_out are host memory.  The box corners lie in [-32768, 32768].
 *
 * Scratch, freed before the call returns: about 24 bytes per source entry (vxrt_edit_voxels_device's front), 8 bytes per block of
 * 2 048 destination cells and about 24 bytes per voxel of the result.  Nothing grows per destination cell.  All scratch is allocated
 * before an output byte is written.
 *
 * Checked in this order:
 *   VXRT_E_INVALID  null context; n >= 2^32 (before any pointer is looked at); null pull, n_out, box_min or box_max;
 *                   pull->reserved != 0 or an entry of m or t beyond its limit; a box corner outside [-32768, 32768]; a box of 2^32
 *                   cells or more; n > 0 with null pos; out_pos without out_mrgb or out_mrgb without out_pos when mrgb is given,
 *                   out_mrgb without mrgb
 *   empty box, n == 0   returns 0 with *n_out = 0 without touching a device pointer
 *   VXRT_E_INVALID  an array that hipPointerGetAttributes does not report as device memory of the context's device, or that ends
 *                   past its allocation
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *   VXRT_E_INVALID  arrays given and cap < the count (*n_out is the count)
 * A refused call writes nothing, and vxrt_last_error says why. */
int vxrt_transform_voxels_device(vxrt_ctx* ctx,
                                 const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n,
                                 const vxrt_affine* pull,
                                 const int32_t box_min[3], const int32_t box_max[3],
                                 int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_TRANSFORM_H */
