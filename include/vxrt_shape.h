/*
 * vxrt_shape.h — a box, ball, cylinder or capsule rasterised into a voxel list in device memory: the optional extension of
 * libvxrt.so for hosts that carve and build with shapes.  A crater is a ball to clear, a tunnel or a beam between two points a
 * capsule, a pillar a cylinder, a wall or a stamp mask a box, turned; an ellipsoid is a ball under a scaling map.  The result goes to
 * vxrt_clear_voxels_device, vxrt_edit_voxels_device, vxrt_set_voxels_device, vxrt_combine_voxels_device (vxrt_setops.h) or
 * vxrt_lookup_voxels_device (the collision test) without a round trip through the host, and the same call gives the same bytes on
 * every device.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status.
 *
 * The shape sits in SHAPE SPACE, at the origin with its axis along z, and every cell of a destination box asks whether its centre,
 * pulled through a fixed-point affine map (vxrt_transform.h's vxrt_affine, with the same limits), lies in it.  The rule is exact and
 * does not depend on schedule, device or call:
 *   1. for a destination cell d of the half-open box [box_min, box_max), per axis i:  P_i = sum_j m[i][j] * (2 d_j + 1) + 2 t[i]  in
 *      64 bits: the pulled centre  M (d + 1/2) + t  in units of 2^-17 cell, vxrt_transform.h's sum of rule 2 before its shift.  The
 *      limits on m and t keep |P_i| under 2^43, so no sum wraps
 *   2. a cell with any |P_i| >= 2^31 is outside; the test is made on the 64-bit values before anything is squared or narrowed, so
 *      a centre pulled far away is absent, never wrapped.  With the limits on r and h no shape reaches that far (8192 cells in
 *      shape space)
 *   3. with R = 2 r and H_i = 2 h[i] as 64-bit integers, d is in the result exactly when
 *        VXRT_SHAPE_BOX       -H_i <= P_i < H_i  on all three axes (half-open: abutting boxes tile)
 *        VXRT_SHAPE_BALL      P_0^2 + P_1^2 + P_2^2 <= R^2
 *        VXRT_SHAPE_CYLINDER  P_0^2 + P_1^2 <= R^2  and  -H_2 <= P_2 < H_2
 *        VXRT_SHAPE_CAPSULE   P_0^2 + P_1^2 + (P_2 - q)^2 <= R^2  with  q = clamp(P_2, -H_2, H_2)
 *      the sums of squares taken in unsigned 64 bits: after rule 2 each square is below 2^62, so three of them do not wrap, and
 *      R^2 <= 2^60
 *   4. with mrgb every voxel of the result carries (mrgb[0] & 0x7f, r, g, b), as vxrt_get_voxels returns them; mrgb == NULL means
 *      positions only, and out_mrgb must then be NULL too; with mrgb, out_pos and out_mrgb come both or neither
 *   5. the result is written in ascending path order at depth 15, the order every device list of this library has (vxrt_extract.h),
 *      each cell once; out_pos == out_mrgb == NULL counts only, and cap is ignored; with arrays and more voxels than cap, *n_out is
 *      the count, nothing is written and the call returns VXRT_E_INVALID
 *   6. an empty box (box_min[i] >= box_max[i] on any axis) gives *n_out = 0 without touching a device pointer
 *
 * A pull map for a shape.  In the coordinates in which cell c is the cube [c, c + 1)^3, a shape with centre p and orientation R (a
 * rotation whose third column is the shape's axis) and a gain g_i >= 1 per shape axis (1 for a rigid shape; an ellipsoid with radii
 * a_i is a ball of radius rho >= max a_i under g_i = rho / a_i) has the pull
 *      m[i][j] = rint(65536 * g_i * R[j][i])
 *      t[i]    = rint(-65536 * g_i * sum_j R[j][i] * p_j)
 * in double precision with rint() of <math.h>.  The destination box is the forward bounding box of the shape, grown by 2 cells per
 * side and clipped to [-32768, 32768]: the rounding of m, at most 2^-17 per entry times a coordinate below 2^15, three terms, moves
 * a pulled centre by up to three quarters of a shape-space cell per axis and the rounding of t by 2^-17 more, under 1.3 cells in
 * length, and with no gain below 1 that is no shorter in the destination; so a cell of the result has its centre within 1.3 cells
 * of the true shape's bounding box, and lies within 1.8 cells of it.
 *
 * The call needs no loaded scene and touches none.
 *
 * Ordering: the arrays are written on the context's stream, behind everything enqueued there; a consumer on another stream orders
 * itself with vxrt_stream_wait_context, and memory that another stream still uses is ordered first with
 * vxrt_context_wait_stream(ctx, that_stream).  The call is synchronous: it waits for its own result, so the arrays may be read,
 * freed or rewritten when it returns.  Two calls with the same arguments write the same bytes.
 *
 * Multi-GPU: call on each rank's context, in its own device's memory.
 */
#ifndef VXRT_SHAPE_H
#define VXRT_SHAPE_H

#include "vxrt_transform.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vxrt_shape_kind { VXRT_SHAPE_BOX = 0, VXRT_SHAPE_BALL = 1, VXRT_SHAPE_CYLINDER = 2, VXRT_SHAPE_CAPSULE = 3 } vxrt_shape_kind;

typedef struct vxrt_shape {
    uint32_t kind;        /* vxrt_shape_kind */
    uint32_t r;           /* Q16 cells, <= 2^29: BALL, CYLINDER, CAPSULE; 0 for BOX */
    uint32_t h[3];        /* Q16 cells, each <= 2^29: BOX half extents; CYLINDER and CAPSULE use h[2] (axis = shape z), h[0] = h[1] = 0; BALL all 0 */
    uint32_t reserved[3]; /* must be 0 */
} vxrt_shape;             /* 32 bytes; host memory */

#ifdef __cplusplus
static_assert(sizeof(vxrt_shape) == 32, "vxrt_shape");
#else
typedef char vxrt_shape_is_32_bytes[sizeof(vxrt_shape) == 32 ? 1 : -1];
#endif

/* out_pos[0 .. cap) and out_mrgb[0 .. cap) are device memory of the context's device and may have any alignment; shape, pull,
 * box_min, box_max, mrgb (4 bytes) and n_out are host memory.  The box corners lie in [-32768, 32768].
 *
 * Scratch, freed before the call returns: about 16 bytes per aligned 16^3 tile of cells that meets the box, and the tile sort's digit
 * counts.  Nothing grows per destination cell or per voxel of the result.  All scratch is allocated before an output byte is written.
 *
 * Checked in this order:
 *   VXRT_E_INVALID  null context; null shape, pull, n_out, box_min or box_max; pull->reserved != 0 or an entry of m or t beyond
 *                   its limit; shape->kind > 3, r or an entry of h beyond 2^29, a field the kind does not use that is not 0,
 *                   shape->reserved != 0; a box corner outside [-32768, 32768]; a box of 2^32 cells or more; out_pos without
 *                   out_mrgb or out_mrgb without out_pos when mrgb is given, out_mrgb without mrgb
 *   empty box       returns 0 with *n_out = 0 without touching a device pointer
 *   VXRT_E_INVALID  an array that hipPointerGetAttributes does not report as device memory of the context's device, or that ends
 *                   past its allocation
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *   VXRT_E_INVALID  arrays given and cap < the count (*n_out is the count)
 * A refused call writes nothing, and vxrt_last_error says why. */
int vxrt_shape_voxels_device(vxrt_ctx* ctx, const vxrt_shape* shape, const vxrt_affine* pull,
                             const int32_t box_min[3], const int32_t box_max[3],
                             const uint8_t mrgb[4],
                             int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_SHAPE_H */
