/*
 * vxrt_pieces.h — per connected component of a voxel list its size, bounding box, coordinate sums and number, and the detached
 * pieces of the loaded scene, piece by piece: the optional extension of libvxrt.so on top of vxrt_components.h.  That header
 * answers "which voxels fell off"; this one answers "which pieces fell off, and how big is each", so a host can turn a piece of 3
 * voxels into particles, one of 300 into a rigid body with a mass, a centre and a box, and leave one of 300 000 where it is.  A host
 * that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status.
 *
 * The rule continues rules 1 to 5 of vxrt_components.h.  It is exact and does not depend on schedule, device or call:
 *   6. components are numbered 0 .. k-1 by ascending label, a label being the least input index in the component; id[i] is the
 *      number of i's component
 *   7. info[c].first is component c's label
 *   8. voxels, min, max and sum are taken over the distinct positions of the component: a position listed four times counts once
 *   9. reserved is 0
 *
 * Multi-GPU: every rank holds the whole scene; call on each rank's context, in its own device's memory.
 */
#ifndef VXRT_PIECES_H
#define VXRT_PIECES_H

#include "vxrt.h"
#include "vxrt_components.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vxrt_piece {
    uint32_t first;     /* see each call */
    uint32_t voxels;    /* distinct positions in the component */
    int16_t  min[3];    /* least coordinate per axis, inclusive */
    int16_t  max[3];    /* greatest coordinate per axis, inclusive */
    uint32_t reserved;  /* written as 0 */
    int64_t  sum[3];    /* sum of each coordinate over the distinct positions: centroid = sum / voxels */
} vxrt_piece;           /* 48 bytes, 8-byte aligned */

#ifdef __cplusplus
static_assert(sizeof(vxrt_piece) == 48 && alignof(vxrt_piece) == 8, "vxrt_piece");
#else
typedef char vxrt_piece_is_48_bytes[sizeof(vxrt_piece) == 48 ? 1 : -1];
typedef char vxrt_piece_is_8_byte_aligned[(sizeof(struct { char c; vxrt_piece p; }) - sizeof(vxrt_piece)) == 8 ? 1 : -1];
#endif

/* The table of the components of a list: vxrt_label_components_device's labelling, and with it id[0 .. n) (rule 6) and
 * info[0 .. *n_components) (rules 7 to 9).  pos, n, connectivity and label are vxrt_label_components_device's, and label, where given,
 * receives exactly the bytes that call writes.  label, id and info may each be NULL; with all three NULL the call counts only.
 * All arrays are device memory of the context's device; label and id are 4-byte aligned, info is 8-byte aligned, pos may have any
 * alignment.  info has room for info_cap entries: with info given and more components than info_cap, *n_components is the count,
 * nothing is written, to label and id neither, and the call returns VXRT_E_INVALID.  n == 0 gives *n_components == 0 without
 * touching a pointer.  No scene is needed and none is touched; pos is never written.
 *
 * Ordering as vxrt_label_components_device: on the context's stream, behind everything enqueued there; the call is synchronous.  Two
 * calls on the same list write the same bytes.
 *
 * Scratch, freed before the call returns: about 40 bytes per entry (the labelling's, two of whose arrays are used again once the
 * labelling is done with them) and, unless the call only counts or only labels, 64 bytes per component.  Every scratch allocation
 * happens before a byte of label, id or info is written.
 *
 *   VXRT_E_INVALID  null context or n_components; n > 0 with null pos; n >= 2^32 (checked before any pointer is looked at); a
 *                   connectivity other than 6, 18 or 26; an array that hipPointerGetAttributes does not report as device memory of
 *                   the context's device, or that ends past its allocation; a misaligned label, id or info; info given and more
 *                   components than info_cap
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *
 * A refused call writes nothing. */
int vxrt_component_table_device(vxrt_ctx* ctx, const int16_t (*pos)[3], size_t n, uint32_t connectivity,
                                uint32_t* label, uint32_t* id, vxrt_piece* info, size_t info_cap, size_t* n_components);

/* The detached pieces of the loaded scene, as it stands.  A component of the scene (by the rule above, over the whole scene) is
 * selected when it holds no voxel in the half-open anchor box [anchor_min, anchor_max), which is vxrt_detached_voxels_device's rule,
 * and min_voxels <= voxels <= max_voxels; 0 and UINT32_MAX select every detached component, and min_voxels > max_voxels is no error:
 * it selects nothing.  pos and mrgb take the selected components' voxels in ascending path order with the bytes vxrt_get_voxels
 * returns; pieces are numbered by their first voxel in that order; piece[i] is the number of returned voxel i's piece, and info[p]
 * describes piece p, its first being the index in the returned list of the piece's first voxel.  So piece and info are exactly the
 * id and info that vxrt_component_table_device gives for the returned pos at the same connectivity, and with the full size range
 * pos and mrgb are byte for byte vxrt_detached_voxels_device's.
 *
 * Count-only form: pos == mrgb == piece == info == NULL.  Otherwise pos and mrgb come both or neither, and piece and info are each
 * optional.  pos, mrgb and piece have room for cap voxels, info for info_cap pieces; with more voxels than cap where pos or piece
 * is given, or with info given and more pieces than info_cap, *n and *n_pieces are the counts, nothing is written and the call
 * returns VXRT_E_INVALID.  pos and mrgb may have any alignment; piece is 4-byte and info 8-byte aligned.  A scene with no voxel
 * gives *n == *n_pieces == 0.  The call reads scenes in any record order and format, runs on the context's stream, waits for the
 * result, and changes no scene byte, image or history.  vxrt_edit_voxels_device(ctx, pos, NULL, *n) clears the returned list.
 *
 * Scratch, freed before the call returns: about 54 bytes per voxel of the scene (vxrt_detached_voxels_device's) plus 64 bytes per
 * component and two small arrays of scan partials, all of it allocated before an output byte is written.
 *
 *   VXRT_E_INVALID  null context, n, n_pieces or anchor pointer; a connectivity other than 6, 18 or 26; pos without mrgb or mrgb
 *                   without pos; an output array that is not device memory of the context's device or ends past its allocation; a
 *                   misaligned piece or info; too little room (see above)
 *   VXRT_E_NOSCENE  no scene is loaded
 *   VXRT_E_DEVICE   the scratch could not be allocated */
int vxrt_detached_pieces_device(vxrt_ctx* ctx, const int32_t anchor_min[3], const int32_t anchor_max[3], uint32_t connectivity,
                                uint32_t min_voxels, uint32_t max_voxels,
                                int16_t (*pos)[3], uint8_t (*mrgb)[4], uint32_t* piece, size_t cap, size_t* n,
                                vxrt_piece* info, size_t info_cap, size_t* n_pieces);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_PIECES_H */
