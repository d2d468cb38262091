/*
 * vxrt_setops.h — two voxel lists in device memory combined into one: union, intersection, difference, symmetric difference and
 * the delta between two snapshots.  The optional extension of libvxrt.so for hosts that join stamps into a prefab, cut one shape
 * out of another, mask a shape, ask whether two loose pieces share a cell, or keep snapshots and need what changed between them
 * (what undo stores, what a network peer is sent, what vxrt_edit_voxels_device and vxrt_clear_voxels_device replay).  The lists come
 * from vxrt_get_voxels_device, vxrt_detached_pieces_device, vxrt_transform_voxels_device, a voxeliser or the host.  A host that
 * only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status.
 *
 * The rule is exact and does not depend on schedule, device or call:
 *   1. each input is the set of distinct positions of its list; the last entry of a position wins (vxrt_edit_voxels_device's rule,
 *      vxrt_transform.h's rule 1) and its bytes are (mrgb[0] & 0x7f, r, g, b), as vxrt_get_voxels returns them
 *   2. membership and bytes per op are vxrt_list_op's, below.  VXRT_LIST_CHANGED compares leaf words, so bit 7 of the material
 *      byte never makes a voxel "changed".  CHANGED(A, B) to set (vxrt_edit_voxels_device) together with the positions of
 *      DIFFERENCE(A, B) to clear (vxrt_clear_voxels_device) turns a scene holding A into one holding B
 *   3. the result is in ascending path order at depth 15, the order every device list of this library has (vxrt_extract.h,
 *      vxrt_transform.h's rule 4); each position appears once
 *   4. values: the call carries bytes exactly when a_mrgb != NULL (also with na == 0, where a_mrgb is not read).  UNION, XOR and
 *      CHANGED then need b_mrgb when nb > 0; INTERSECT and DIFFERENCE take bytes from A only, so b_mrgb may be NULL, which makes B
 *      a mask, or may be given and is then ignored.  With a_mrgb == NULL, b_mrgb and out_mrgb must be NULL and CHANGED is refused.
 *      With bytes, out_pos and out_mrgb come both or neither
 *   5. out_pos == out_mrgb == NULL counts only, and cap is ignored: counting INTERSECT is the collision test of two lists.  With
 *      arrays and more voxels than cap, *n_out is the count, nothing is written and the call returns VXRT_E_INVALID
 *   6. na == 0 and nb == 0 gives *n_out = 0 without touching a device pointer.  One empty list is legal and its pointers may be
 *      NULL: UNION with an empty B is A deduplicated, in path order
 *   7. every input byte is read before the first output byte is written (the inputs are copied into scratch keys first), so
 *      out_pos / out_mrgb may be either input's arrays
 *
 * The call needs no loaded scene and touches none.
 *
 * Ordering: the arrays are read and written on the context's stream, behind everything enqueued there; a producer on another stream
 * orders itself first with vxrt_context_wait_stream(ctx, producer_stream).  The call is synchronous: it waits for its own result, so
 * the arrays may be freed or rewritten when it returns.  Two calls with the same arguments write the same bytes.
 *
 * Multi-GPU: call on each rank's context, in its own device's memory.
 */
#ifndef VXRT_SETOPS_H
#define VXRT_SETOPS_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vxrt_list_op {
    VXRT_LIST_UNION      = 0,   /* in A or in B;             bytes of B where both have it (A, then B, last wins: the edit rule) */
    VXRT_LIST_INTERSECT  = 1,   /* in A and in B;            bytes of A (A masked by B) */
    VXRT_LIST_DIFFERENCE = 2,   /* in A and not in B;        bytes of A (B cut out of A) */
    VXRT_LIST_XOR        = 3,   /* in exactly one;           its own bytes */
    VXRT_LIST_CHANGED    = 4    /* in B, and absent from A or with a different leaf word there; bytes of B */
} vxrt_list_op;

/* a_pos[0 .. na), a_mrgb[0 .. na), b_pos[0 .. nb), b_mrgb[0 .. nb), out_pos[0 .. cap) and out_mrgb[0 .. cap) are device memory of
 * the context's device and may have any alignment; n_out is host memory.  op is a vxrt_list_op.
 *
 * Scratch, freed before the call returns: about 24 bytes per entry of either list (vxrt_edit_voxels_device's front, run once per
 * list), 8 bytes per block of 2 048 unique entries and 12 bytes per voxel of the result.  All scratch is allocated before an output
 * byte is written.
 *
 * Checked in this order:
 *   VXRT_E_INVALID  null context; na or nb >= 2^32 (before any pointer is looked at); null n_out; op > 4; the values of rule 4;
 *                   na > 0 with null a_pos, nb > 0 with null b_pos
 *   na == 0 and nb == 0   returns 0 with *n_out = 0 without touching a device pointer
 *   VXRT_E_INVALID  an array given (an input of a list with entries, an output) that hipPointerGetAttributes does not report as
 *                   device memory of the context's device, or that ends past its allocation; the outputs at cap entries
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *   VXRT_E_INVALID  the two lists' distinct positions number 2^32 or more together
 *   VXRT_E_INVALID  arrays given and cap < the count (*n_out is the count)
 * A refused call writes nothing, and vxrt_last_error says why. */
int vxrt_combine_voxels_device(vxrt_ctx* ctx,
                               const int16_t (*a_pos)[3], const uint8_t (*a_mrgb)[4], size_t na,
                               const int16_t (*b_pos)[3], const uint8_t (*b_mrgb)[4], size_t nb,
                               uint32_t op, int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], size_t cap, size_t* n_out);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_SETOPS_H */
