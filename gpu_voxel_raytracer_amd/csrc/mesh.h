// mesh.h — what api_mesh.hip (host side of vxrt_mesh.h) and mesh.hip (its kernels) share.  DESIGN.md §27.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "mesh_rule.h"
#include "morph.h"

namespace vxrt {

// Every kernel here runs morph.h's geometry: blocks of kMorphThreads threads over kMorphSpan consecutive entries each, so a grid
// has morph_blocks(count) blocks.  The counting kernels write part[0 .. morph_blocks(count)); the emitting ones read it scanned.

// part[b] = the faces of block b's voxels: the popcount of mesh_face_dirs(masks[i]), masks being launch_morph_mask's at
// connectivity 6.
hipError_t launch_mesh_face_count(const uint32_t* masks, uint32_t m, uint64_t* part, hipStream_t stream);

// Every face of the set (mesh_face_of; the voxel's leaf word beside it where out_words != nullptr) at part[b] onward, in no order
// the caller may rely on but the same one every time.
hipError_t launch_mesh_face_emit(const MorphSet& s, const uint32_t* masks, const uint64_t* part, uint64_t* out_faces, uint32_t* out_words,
                                 hipStream_t stream);

// The run heads (mesh_is_head) of `count` sorted faces (words == nullptr: bytes do not matter).  Counting (out_heads == nullptr):
// part[b] = the heads in block b; a block's first face is compared with the last face of the block before.  Emitting: the heads'
// indices into `faces` at part[b] onward, ascending.
hipError_t launch_mesh_heads(const uint64_t* faces, const uint32_t* words, uint32_t count, uint32_t mode, uint64_t* part, uint32_t* out_heads,
                             hipStream_t stream);

// The four corner keys (mesh_quad_corners) of quad j, which begins at faces[heads[j]] and ends where quad j + 1 begins (the last:
// at `count`), at out_corners[4 j] onward.
hipError_t launch_mesh_quad_corners(const uint64_t* faces, uint32_t count, const uint32_t* heads, uint32_t quads, uint64_t* out_corners,
                                    hipStream_t stream);

// The vertices are the distinct keys among the sorted corner keys: their run heads at shift 0 (run_heads.h).

// The output's writers.  Quad j's corners are looked up among verts[0 .. n_verts) (mesh_corner_index) and its triangles 2 j and
// 2 j + 1 written to out_tris (4-byte aligned), with the quad's bytes to out_mrgb (any alignment) where out_mrgb != nullptr (words
// are then the sorted faces' leaf words).
hipError_t launch_mesh_triangles(const uint64_t* faces, const uint32_t* words, uint32_t count, const uint32_t* heads, uint32_t quads,
                                 const uint64_t* verts, uint32_t n_verts, uint32_t* out_tris, uint8_t* out_mrgb, hipStream_t stream);
// verts[i] as three floats at out_verts[3 i] onward (4-byte aligned).
hipError_t launch_mesh_vertices(const uint64_t* verts, uint32_t n_verts, float* out_verts, hipStream_t stream);

}  // namespace vxrt
