/*
 * vxrt_grid_edit.h — a dense grid in device memory written into a box of a loaded scene, in place: the optional extension of
 * libvxrt.so for hosts that read a box with vxrt_get_voxel_grid (vxrt_grid.h), change it on the GPU (a sculpting brush, a cellular
 * automaton, destruction, a simulation step) and put it back.  A host that only renders needs nothing from here.  Conventions as in
 * vxrt.h: 0 or a negative vxrt_status, host pointers borrowed for the call only.
 *
 * The call diffs the grid against the scene on the device and applies the difference as the in-place edits of vxrt_edit.h: the
 * temporal history is kept, the depth never changes, and nothing but the changed cells is touched.
 *
 * Multi-GPU: every rank holds the whole scene; give each rank's context the same call, with the grid in its own device's memory.
 */
#ifndef VXRT_GRID_EDIT_H
#define VXRT_GRID_EDIT_H

#include "vxrt_grid.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vxrt_grid_edit_mode {
    VXRT_GRID_EDIT_REPLACE = 1, /* every cell of the box becomes the grid's: occupied -> that voxel, empty -> no voxel */
    VXRT_GRID_EDIT_SET = 2,     /* occupied cells are set (insert or overwrite); empty cells leave the scene as it is  */
    VXRT_GRID_EDIT_CLEAR = 3    /* occupied cells are cleared (carve); empty cells leave the scene as it is            */
} vxrt_grid_edit_mode;

typedef struct vxrt_grid_edit_counts {
    uint64_t set;     /* cells set: the length of the sets list below     */
    uint64_t cleared; /* cells cleared: the length of the clears list below */
} vxrt_grid_edit_counts;

/* Write the grid into the box origin + [0, dims) (any int32 box) of the context's scene.  cells, format and palette follow
 * vxrt_set_voxel_grid: device memory of the context's device, dims[0] * dims[1] * dims[2] cells, C order [x][y][z], cell (i, j, k)
 * at position origin + (i, j, k); PALETTE8 cells with a 256-entry host palette (entry 0 ignored), WORD32 cells as leaf words (bit 31
 * set = occupied).
 *
 * With s(p) the scene's leaf word at p (0: no voxel) and g(p) the grid's, over the cells of the box inside the root cube
 * [-2^d, 2^d)^3 (d = vxrt_stats.octree_depth):
 *   clears  the cells with s(p) != 0 that the mode empties (REPLACE: g(p) empty; CLEAR: g(p) occupied)
 *   sets    the cells the mode fills (SET, REPLACE: g(p) occupied) with s(p) != g(p)
 * and the call is exactly vxrt_edit_voxels(clears) followed by vxrt_edit_voxels(sets), each skipped when its list is empty: the same
 * records and leaf words, byte for byte, the same storage growth, sky-cull box, vxrt_stats and frames.  counts (optional) receives
 * the two lengths; when both are 0 nothing is changed.
 *
 * Ordering: synchronous like vxrt_edit_voxels (frames enqueued before the call see the old scene).  The cells are read on the
 * context's stream, behind everything enqueued there (a producer on another stream orders itself first with
 * vxrt_context_wait_stream); they may be rewritten once the call returns.
 * All or nothing — a refused call changes nothing:
 *   VXRT_E_INVALID  null context, dims or origin; null cells with a non-empty box; a bad format or mode; PALETTE8 without a
 *                   palette or WORD32 with one; a box of 2^64 bytes or more; cells that are not device memory of the context's device
 *                   or end past their allocation; a scene with wide records or re-laid as treelets (as vxrt_edit_voxels)
 *   VXRT_E_NOSCENE  no scene set
 *   VXRT_E_SCENE    SET or REPLACE with an occupied cell outside the root cube (empty cells outside it, and every cell outside it
 *                   under CLEAR, are ignored); 2^32 sets or clears or more; an edited scene of 2^32 records or more
 *   VXRT_E_DEVICE   the scratch could not be allocated or the scene's storage could not grow */
int vxrt_edit_voxel_grid(vxrt_ctx* ctx, const void* cells, vxrt_grid_format format, const uint32_t dims[3], const int32_t origin[3],
                         const uint8_t (*palette)[4], vxrt_grid_edit_mode mode, vxrt_grid_edit_counts* counts);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_GRID_EDIT_H */
