/*
 * vxrt_solid.h — a closed triangle mesh in device memory -> the voxels inside it, alone or together with the voxels its surface
 * meets, as a voxel list in device memory: the optional extension of libvxrt.so for hosts that want a mesh as a solid.  The surface
 * list of vxrt_voxelize_mesh_device (vxrt_voxelize.h) is a shell one voxel thick: the first edit that digs into it shows a hollow
 * object, and clearing it carves nothing out of a scene.  The lists from here are what vxrt_set_voxels_device (vxrt_device_scene.h)
 * and vxrt_edit_voxels_device (vxrt_device_edit.h) take: VXRT_SOLID_UNION to set a solid, VXRT_SOLID_INTERIOR (with the surface
 * list, or alone) to clear one.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative
 * vxrt_status.
 *
 * The interior rule is exact integer arithmetic, continuing the rule of vxrt_voxelize.h: coordinates are sixteenths
 * of a voxel, q the snapped vertices, the centre of cell (x, y, c) is (16 x + 8, 16 y + 8, 16 c + 8), and columns run along z for
 * every triangle.
 *   1. a triangle's columns are the cells (x, y) with lo_x <= 16 x + 8 <= hi_x and lo_y <= 16 y + 8 <= hi_y, lo and hi its least and
 *      greatest q; it may have none, and a triangle with n_z == 0 (n = e0 x e1) is skipped
 *   2. a column is under the triangle iff an odd number of its three edges count in the xy-projection, p = (16 x + 8, 16 y + 8): an
 *      edge a b counts iff (a_y <= p_y) != (b_y <= p_y) and, with l, u its ends ordered so that l_y <= p_y < u_y,
 *      (u_x - l_x)(p_y - l_y) - (p_x - l_x)(u_y - l_y) > 0.  The test does not depend on the edge's direction, so two triangles that
 *      share an edge agree on it, and a centre exactly on a projected edge or vertex belongs to exactly one side
 *   3. the triangle crosses such a column at k = floor(-sign(n_z) A / (16 |n_z|)) + 1, A = n . ((16 x + 8, 16 y + 8, 8) - q_0): the
 *      least cell whose centre lies strictly above the triangle's plane (a centre exactly on the plane is below)
 *   4. with a column's crossings sorted, k_0 <= k_1 <= ..., its interior cells are c in [k_2i, k_2i+1)
 *   5. a column with an odd number of crossings means the mesh is not closed, and the call refuses.  A mesh in which every edge
 *      belongs to an even number of triangles never refuses, whatever degenerate or vertical triangles it holds
 * This is parity, not winding: the orientation of the triangles does not matter, overlapping closed shells XOR (the cells inside
 * both are outside), and a shell inside a shell is a cavity.
 *
 * Multi-GPU: every rank holds the whole scene; voxelise on each rank's context, in its own device's memory.
 */
#ifndef VXRT_SOLID_H
#define VXRT_SOLID_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    VXRT_SOLID_UNION = 0,    /* the surface's voxels and the interior cells the surface does not meet */
    VXRT_SOLID_INTERIOR = 1  /* the interior cells and nothing else */
} vxrt_solid_mode;

/* The mesh (verts, n_verts, tris, tri_mrgb, n_tris), pos, mrgb, cap and n: as vxrt_voxelize_mesh_device takes them, with the same
 * pointer checks, snapping, stream ordering (the mesh is read on the context's stream; the call is synchronous), count-only form
 * (pos == mrgb == NULL), cap rule and determinism: two calls on the same mesh write the same bytes.  No scene is needed and none is
 * touched.  n_tris == 0 gives *n == 0 without touching a pointer.  fill_mrgb is host memory: one (material, r, g, b).
 *
 *   VXRT_SOLID_INTERIOR  the interior cells of the rule above, each with the bytes (fill_m & 0x7f, r, g, b).  tri_mrgb may be NULL.
 *                        Cleared from a scene (vxrt_edit_voxels_device without words), this list carves the shape out of it.
 *   VXRT_SOLID_UNION     the voxels of vxrt_voxelize_mesh_device on the same mesh, the same cells with the same bytes, and the
 *                        interior cells that are not among them, with the fill bytes.  tri_mrgb is required with output arrays.
 * The result is unique voxels in ascending path order (the order of vxrt_get_voxels, vxrt_extract.h).
 *
 * Scratch, freed before the call returns: 64 bytes per triangle, 16 bytes per crossing (a pair of a triangle and a column under it),
 * and per list entry (an interior cell, or a triangle-cell overlap of the surface) about 24 bytes (16 when only counting).  Every
 * scratch allocation happens before an output byte is written.
 *
 *   VXRT_E_INVALID  everything vxrt_voxelize_mesh_device refuses as invalid; mode other than the two above; output arrays with
 *                   fill_mrgb NULL, or in VXRT_SOLID_UNION mode with tri_mrgb NULL
 *   VXRT_E_SCENE    a vertex out of range, as in vxrt_voxelize_mesh_device; the mesh is not closed (vxrt_last_error names the first
 *                   column (x, y), in x, then y order, with an odd number of crossings, and that number); the z-columns of all
 *                   triangles, the crossings, or the list's entries (the interior cells, and in VXRT_SOLID_UNION mode the surface's
 *                   triangle-cell overlaps with them) reach 2^32 (vxrt_last_error gives the figures)
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *
 * A refused call writes nothing to pos and mrgb; *n is set only on success and on cap < the count. */
int vxrt_voxelize_solid_device(vxrt_ctx* ctx, const float (*verts)[3], size_t n_verts, const uint32_t (*tris)[3],
                               const uint8_t (*tri_mrgb)[4], size_t n_tris, const uint8_t fill_mrgb[4] /* host memory */,
                               uint32_t mode, int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_SOLID_H */
