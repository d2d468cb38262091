/*
 * vxrt_grid.h — scenes from dense voxel grids in device memory, and boxes of a scene written back as dense grids: the optional
 * extension of libvxrt.so for hosts whose voxels live in a 3-D volume on the GPU (an occupancy or palette-index volume, a thresholded
 * SDF, a cellular automaton, a .vox-style index grid).  A host that only renders needs nothing from here.  Conventions as in vxrt.h:
 * 0 or a negative vxrt_status, host pointers borrowed for the call only.
 *
 * The import walks the grid in aligned 16^3 tiles: taken in Morton order, their occupied cells are already in octree path order, so
 * the octree is built from them without the list builder's sort.  Every position is a prefix sum, so two calls on
 * the same grid write the same bytes.
 *
 * Multi-GPU: every rank holds the whole scene; give each rank's context the grid in its own device's memory.
 */
#ifndef VXRT_GRID_H
#define VXRT_GRID_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vxrt_grid_format {
    VXRT_GRID_PALETTE8 = 1, /* uint8 cells: 0 = empty; i = 1..255 = a voxel with palette[i] as its (material, r, g, b) */
    VXRT_GRID_WORD32 = 2    /* uint32 cells: bit 31 set = a voxel whose leaf word IS the cell
                               (0x80000000 | (m & 0x7f) << 24 | r << 16 | g << 8 | b); bit 31 clear = empty (other bits ignored) */
} vxrt_grid_format;

/* The scene of a dense grid.  cells: device memory of the context's device, dims[0] * dims[1] * dims[2] cells of the format, C order
 * [x][y][z] (z fastest); cell (i, j, k) is the voxel at position origin + (i, j, k) in vxrt_set_voxels coordinates.  palette: host
 * memory, 256 entries (entry 0 ignored), VXRT_GRID_PALETTE8 only; NULL for VXRT_GRID_WORD32.
 *
 * The result is exactly what vxrt_set_voxels of the occupied cells as a list does to the context: the same 8-byte records and leaf
 * words, byte for byte, the same depth, sky-cull box and vxrt_stats, the same VXRT_OPT_NODE_ORDER and VXRT_OPT_SCENE_FORMAT
 * handling, the same frames; the temporal history is reset.  An all-empty grid, or a zero dim, gives the empty scene.
 *
 * Ordering: the call reads the cells on the context's stream, behind everything enqueued there (a producer on another stream orders
 * itself first with vxrt_context_wait_stream).  The call is synchronous: the cells may be rewritten once it returns.
 *
 *   VXRT_E_INVALID  null context, dims or origin; null cells with a non-empty grid; a bad format; PALETTE8 without a palette or
 *                   WORD32 with one; cells that are not device memory of the context's device or end past their allocation; a box
 *                   outside the int16 range (origin < -32768 or origin + dims > 32768 on some axis)
 *   VXRT_E_SCENE    2^32 occupied cells or more, or 2^32 records or more
 *   VXRT_E_DEVICE   the scratch or the new scene could not be allocated
 *
 * A refused call changes nothing: the previous scene stays, byte for byte, and renders as before. */
int vxrt_set_voxel_grid(vxrt_ctx* ctx, const void* cells, vxrt_grid_format format, const uint32_t dims[3], const int32_t origin[3],
                        const uint8_t (*palette)[4]);

/* The scene as it stands after everything enqueued so far (edits included), written as VXRT_GRID_WORD32 cells for the box
 * origin + [0, dims) (any int32 box) into cells, device memory of the context's device, C order [x][y][z]: the leaf word of every
 * voxel, 0 for every empty cell and every cell outside the root cube.  Reads every layout of the records (vxrt_extract.h).
 *
 * The call is enqueued on the context's stream and returns without waiting; a consumer on another stream orders itself with
 * vxrt_stream_wait_context.  It changes no scene byte, no image and no temporal history.
 *
 *   VXRT_E_INVALID  null context, origin or dims; null cells with a non-empty box; a box of 2^64 bytes or more; cells that are not
 *                   device memory of the context's device or end past their allocation
 *   VXRT_E_NOSCENE  no scene set */
int vxrt_get_voxel_grid(vxrt_ctx* ctx, const int32_t origin[3], const uint32_t dims[3], uint32_t* cells);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_GRID_H */
