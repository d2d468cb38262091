/*
 * vxrt_mesh.h — a voxel list in device memory as an indexed triangle mesh of its exposed faces.  The optional extension of
 * libvxrt.so for hosts that hand a detached piece to a physics engine or a rasteriser as debris, export an edited scene, or show a
 * collision hull: the way back out of the voxel lists that vxrt_voxelize_mesh_device and vxrt_voxelize_solid_device lead into.
 * The list comes from vxrt_get_voxels_device, vxrt_detached_pieces_device, vxrt_transform_voxels_device,
 * vxrt_combine_voxels_device, vxrt_morph_voxels_device, a voxeliser or the host.  The inside of a solid contributes no face and
 * never leaves the device.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative vxrt_status.
 *
 * The rule is exact and does not depend on schedule, device or call:
 *   1. the input S is the set of distinct positions of the list; the last entry of a position wins and its bytes are
 *      (mrgb[0] & 0x7f, r, g, b): rule 1 of vxrt_morph.h
 *   2. faces.  Directions d = 0 .. 5 are the first six rows of vxrt_morph.h's offset table: -x, -y, -z, +z, +y, +x.  A voxel p of S
 *      has a face in direction d iff p + o_d is not in S; a neighbour outside the int16 range is not in S, so a voxel on the
 *      range's edge shows that face.  With a the normal's axis and s its sign, b = (a + 1) mod 3 and c = (a + 2) mod 3, the face is
 *      the unit square at w = p_a + (s > 0 ? 1 : 0) on axis a, over [p_b, p_b + 1] x [p_c, p_c + 1].  Its face key is
 *      (d, w, p_b, p_c), compared in that order (3 + 17 + 16 + 16 bits with the coordinates offset by 32768)
 *   3. quads.  In VXRT_MESH_FACES mode every face is a quad.  In VXRT_MESH_RUNS mode a face joins the quad of its predecessor in
 *      ascending face-key order iff it has the same d, w and p_b, its p_c is the predecessor's p_c + 1, and it has the same four
 *      bytes; in a call without mrgb, bytes do not matter.  So runs extend along z for x-normals, along x for y-normals and along y
 *      for z-normals, and have any length.  A quad is [b0, b1] x [c0, c1] with b1 = b0 + 1.  Quads are emitted in ascending
 *      face-key order of their first face, in both modes
 *   4. corners and triangles.  With P(b, c) the point whose axis a is w, the corners k0 .. k3 for s > 0 are P(b0, c0), P(b1, c0),
 *      P(b1, c1), P(b0, c1), and for s < 0 P(b0, c0), P(b0, c1), P(b1, c1), P(b1, c0): counter-clockwise seen from outside.
 *      Quad j gives triangles 2 j = (k0, k1, k2) and 2 j + 1 = (k0, k2, k3); both carry the voxel's bytes in out_tri_mrgb
 *   5. vertices are the distinct corners of all quads, each once, ascending by (x, y, z), written as binary32 (integers up to
 *      32768 are exact).  out_tris holds indices into that array; no vertex is unused
 *   6. values: with mrgb == NULL, out_tri_mrgb must be NULL.  With mrgb, out_tri_mrgb comes iff out_tris does.  out_verts and
 *      out_tris come both or neither
 *   7. out_verts == out_tris == NULL counts only, and the caps are ignored.  With arrays, if either count exceeds its cap, both
 *      counts are set, nothing is written and the call returns VXRT_E_INVALID.  n == 0 gives 0 / 0 without touching a device
 *      pointer.  A host can size without counting: there are at most 12 triangles and 8 vertices per list entry
 *   8. every input byte is read before the first output byte is written (the input is copied into scratch keys first), so
 *      out_tri_mrgb may be the input's mrgb
 *
 * What follows from the rule:
 *   - the mesh is closed in the sense of vxrt_solid.h: vxrt_voxelize_solid_device(..., VXRT_SOLID_INTERIOR) of it returns exactly
 *     S, in both modes, provided no voxel coordinate is 32767 (a voxel there has a vertex at 32768, which the voxelisers refuse)
 *   - in RUNS mode the mesh has T-junctions: a long quad lies beside unit quads whose corners are on its edge.  The solid rule's
 *     edge test is exact on collinear sub-edges, so the round trip holds all the same; a consumer that needs a watertight
 *     edge-to-edge mesh takes FACES mode
 *   - in FACES mode every edge belongs to an even number of triangles
 *
 * The outputs are what vxrt_voxelize_mesh_device and vxrt_voxelize_solid_device take as verts, tris and tri_mrgb.  The call needs
 * no loaded scene and touches none.
 *
 * Ordering: the arrays are read and written on the context's stream, behind everything enqueued there; a producer on another stream
 * orders itself first with vxrt_context_wait_stream(ctx, producer_stream).  The call is synchronous: it waits for its own result, so
 * the arrays may be freed or rewritten when it returns; it does not call vxrt_sync.  Two calls with the same arguments write the
 * same bytes.
 *
 * Multi-GPU: call on each rank's context, in its own device's memory.
 */
#ifndef VXRT_MESH_H
#define VXRT_MESH_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum vxrt_mesh_mode {
    VXRT_MESH_FACES = 0,   /* every exposed face is a quad: two triangles per face */
    VXRT_MESH_RUNS  = 1    /* consecutive faces of one row and one colour share a quad */
} vxrt_mesh_mode;

/* pos[0 .. n), mrgb[0 .. n), out_verts[0 .. vert_cap), out_tris[0 .. tri_cap) and out_tri_mrgb[0 .. tri_cap) are device memory of
 * the context's device; out_verts and out_tris are 4-byte aligned, the others may have any alignment; n_verts and n_tris are host
 * memory.  mode is a vxrt_mesh_mode.
 *
 * Scratch, freed before the call returns: about 24 bytes per entry of the list (vxrt_edit_voxels_device's front) and 4 per voxel;
 * about 16 bytes per face, 24 with bytes (the face keys and leaf words, double-buffered for the sort); per quad 4 bytes and about
 * 64 for its four corner keys, double-buffered; 8 bytes per vertex.  Every allocation is made before the launches that use it, and
 * the two kernels that write the output run last.
 *
 * Checked in this order:
 *   VXRT_E_INVALID  null context; n >= 2^32 (before any pointer is looked at); null n_verts or n_tris; mode > 1; the values of
 *                   rule 6; n > 0 with null pos
 *   n == 0          returns 0 with *n_verts = *n_tris = 0 without touching a device pointer
 *   VXRT_E_INVALID  an array given that hipPointerGetAttributes does not report as device memory of the context's device, or that
 *                   ends past its allocation (the outputs at their caps); out_verts or out_tris not 4-byte aligned
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *   VXRT_E_INVALID  2^32 faces or more, or 2^30 quads or more
 *   VXRT_E_INVALID  arrays given and vert_cap < *n_verts or tri_cap < *n_tris (both counts are set)
 * A refused call writes nothing, and vxrt_last_error says why. */
int vxrt_mesh_voxels_device(vxrt_ctx* ctx, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, uint32_t mode,
                            float (*out_verts)[3], size_t vert_cap,
                            uint32_t (*out_tris)[3], uint8_t (*out_tri_mrgb)[4], size_t tri_cap,
                            size_t* n_verts, size_t* n_tris);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_MESH_H */
