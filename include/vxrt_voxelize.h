/*
 * vxrt_voxelize.h — a triangle mesh in device memory -> the voxels its surface meets, as a voxel list in device memory: the optional
 * extension of libvxrt.so for hosts whose content is a mesh (a simulation's surface, an asset, a brush shaped like an object).  The
 * list is what vxrt_set_voxels_device (vxrt_device_scene.h) and vxrt_edit_voxels_device (vxrt_device_edit.h) take, so a mesh reaches
 * the scene without crossing to the host.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a
 * negative vxrt_status.
 *
 * The rule is exact integer arithmetic, so the result does not depend on the device, the schedule or the call:
 *   1. a vertex is snapped to sixteenths of a voxel, q = rint(16 v) in binary32, ties to even; the voxel at integer position p is
 *      the cube [p, p + 1)^3, sixteenths [16 p, 16 p + 16)
 *   2. per triangle and axis, with lo and hi the least and greatest q, the candidate cells are floor(lo / 16) <= c <=
 *      (hi == lo ? floor(lo / 16) : ceil(hi / 16) - 1): a face lying exactly on a cell boundary belongs to the cell above it only
 *   3. a candidate cell is set when the other ten axes of the Akenine-Moller triangle-box test find no separation between the
 *      snapped triangle and the cell's cube; touching counts as overlap.  A triangle that is a segment or a point takes the same
 *      tests and sets the cells the segment or point meets
 *   4. a voxel that several triangles set takes the mrgb of the highest triangle index
 * Interiors are not filled here (vxrt_solid.h fills them), and there are no vertex transforms or textures.
 *
 * Multi-GPU: every rank holds the whole scene; voxelise on each rank's context, in its own device's memory.
 */
#ifndef VXRT_VOXELIZE_H
#define VXRT_VOXELIZE_H

#include "vxrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* verts[0 .. n_verts), in voxel units; tris[0 .. n_tris), three vertex indices each; tri_mrgb[0 .. n_tris), one (material, r, g, b)
 * per triangle; pos and mrgb: the result.  All five arrays are device memory of the context's device (hipMalloc, or a torch tensor's
 * storage); verts and tris are 4-byte aligned, the others may have any alignment.
 *
 * The result is the mesh's voxels, each once, in ascending path order (the order of vxrt_get_voxels, vxrt_extract.h), with the bytes
 * (m & 0x7f, r, g, b) that vxrt_get_voxels returns.  pos == mrgb == NULL counts only (tri_mrgb may then be NULL too).  With arrays,
 * cap is their room in voxels: when the mesh gives more, *n is the count, nothing is written and the call returns VXRT_E_INVALID.
 * n_tris == 0 gives *n == 0.
 *
 * The call reads and writes no scene byte, image or history, and needs no scene.  It reads the mesh on the context's stream, behind
 * everything enqueued there; a producer on another stream orders itself first with vxrt_context_wait_stream(ctx, producer_stream).
 * The call is synchronous: it returns when the list is written, and the mesh may be freed or rewritten from then on.  Two calls on
 * the same mesh write the same bytes.
 *
 * Scratch, freed before the call returns: 56 bytes per triangle, and per triangle-cell overlap found (a voxel that k triangles meet
 * counts k times) about 24 bytes (16 when only counting).  Every scratch allocation happens before an output byte is written.
 *
 *   VXRT_E_INVALID  null context or n; pos without mrgb or mrgb without pos; output arrays without tri_mrgb; n_tris >= 2^32; an
 *                   array that hipPointerGetAttributes does not report as device memory of the context's device (pageable, pinned
 *                   or managed host memory included), that ends past its allocation, or verts / tris not 4-byte aligned; a
 *                   triangle index >= n_verts; a vertex that a triangle uses and that is not finite (unused vertices are never
 *                   read); cap < the count
 *   VXRT_E_SCENE    a vertex that a triangle uses snaps outside [-2^19, 2^19) sixteenths, that is outside [-32768, 32768) voxels
 *                   (vxrt_last_error gives the bounds and the mesh's span); the candidate columns of all triangles (per triangle,
 *                   the product of its cell ranges on the two axes other than the first axis of greatest |normal component|) or the
 *                   triangle-cell overlaps before the dedupe reach 2^32 (vxrt_last_error gives both figures)
 *   VXRT_E_DEVICE   the scratch could not be allocated
 *
 * A refused call writes nothing to pos and mrgb; *n is set only on success and on cap < the count. */
int vxrt_voxelize_mesh_device(vxrt_ctx* ctx, const float (*verts)[3], size_t n_verts, const uint32_t (*tris)[3],
                              const uint8_t (*tri_mrgb)[4], size_t n_tris, int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap, size_t* n);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_VOXELIZE_H */
