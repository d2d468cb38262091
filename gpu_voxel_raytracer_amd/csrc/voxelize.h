// voxelize.h — what api_voxelize.hip (host side of vxrt_voxelize.h) and voxelize.hip (its kernels) share.  DESIGN.md §17.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ctx.h"

namespace vxrt {

// A work item is one (triangle, column) pair: a column is a line of candidate cells along the first axis of greatest |n_a| of the
// triangle's normal, so a triangle has as many columns as its cell ranges on the other two axes multiply to.  Items are numbered in
// triangle order, then column order; every output position is a prefix sum over that numbering, never an atomic.
constexpr uint32_t kVoxThreads = 256;        // every kernel here; also the triangles per block of the setup pass and the items per block of the walk

constexpr uint32_t kVoxBadIndex = 1u;        // MeshSummary::flags: a triangle names a vertex >= n_verts
constexpr uint32_t kVoxNotFinite = 2u;       //                     a used vertex is NaN or infinite
constexpr uint32_t kVoxOutside = 4u;         //                     a used vertex snaps outside [-2^19, 2^19) sixteenths

constexpr int32_t kVoxSnapLo = -(1 << 19), kVoxSnapHi = 1 << 19;

// A triangle's vertices snapped to sixteenths of a voxel, q[3 * k + axis] (zeros for a triangle that raised a flag).
struct VoxTri {
    int32_t q[9];
    uint32_t pad[3];
};
static_assert(sizeof(VoxTri) == 48, "three 16-byte loads");

// The mesh as the setup pass saw it: the candidate cells' least and greatest coordinate per axis over all triangles (cells of the
// snapped vertices clamped to +-2^26 where one lies outside), and the flags above.
struct MeshSummary {
    int32_t lo[3], hi[3];
    uint32_t flags, pad;
};

inline uint32_t vox_blocks(uint64_t n) { return uint32_t((n + kVoxThreads - 1) / kVoxThreads); }

// the exact integer arithmetic of the rules on snapped coordinates (voxelize.hip, solid.hip)
__device__ __forceinline__ int64_t wmul(int a, int b) { return int64_t(a) * int64_t(b); }
__device__ __forceinline__ int min3(int a, int b, int c) { return min(a, min(b, c)); }
__device__ __forceinline__ int max3(int a, int b, int c) { return max(a, max(b, c)); }

// The setup pass over n_tris > 0 triangles (< 2^32): tq[t] = triangle t snapped, off[t] = the columns of the triangles before t,
// off[n_tris] = *columns = all columns (W), *out = the summary.  part: vox_blocks(n_tris) + 1 words, bounds: vox_blocks(n_tris) + 1
// summaries.  No index is followed before it is compared with n_verts.  Waits for the result; with a flag set, off is meaningless.
int voxelize_setup(const float* verts, size_t n_verts, const uint32_t* tris, size_t n_tris, VoxTri* tq, uint64_t* off, uint64_t* part,
                   MeshSummary* bounds, hipStream_t stream, MeshSummary* out, uint64_t* columns);

// The walk over the columns items (0 < columns < 2^32), counting: part[b] = the hits of items [256 b, 256 b + 256) scanned
// exclusively, part[vox_blocks(columns)] = *hits = all of them.  Waits for the result.
int voxelize_count(const VoxTri* tq, const uint64_t* off, uint32_t n_tris, uint32_t columns, uint64_t* part, hipStream_t stream,
                   uint64_t* hits);

// The same walk, writing hit h's path key at `depth` (device_build.h: path_key_of) to keys[h] and, with vals, the leaf word of its
// triangle's tri_mrgb to vals[h]; h runs in item order and, within an item, up the column.  part: as voxelize_count left it.
hipError_t voxelize_emit(const VoxTri* tq, const uint64_t* off, uint32_t n_tris, uint32_t columns, const uint64_t* part, uint32_t depth,
                         const uint8_t* tri_mrgb, uint64_t* keys, uint32_t* vals, hipStream_t stream);

// m path keys at `depth` and their leaf words -> positions (3 int16 each, pos 2-byte aligned) and (m & 0x7f, r, g, b) bytes (mrgb
// 4-byte aligned), as vxrt_get_voxels gives them.
hipError_t voxelize_decode(const uint64_t* keys, const int32_t* words, uint32_t m, uint32_t depth, int16_t* pos, uint32_t* mrgb,
                           hipStream_t stream);

// ---- api_voxelize.hip: what the entry points that take a mesh share (vxrt_voxelize_mesh_device, vxrt_voxelize_solid_device)
// The checks of a mesh's arrays and of the output arrays, n_tris > 0: null and misaligned pointers, then check_device_array on each
// array given (tri_mrgb may be null; pos and mrgb are looked at when pos is not null and cap != 0).  who: the API call.
int voxelize_check_args(vxrt_ctx* c, const char* who, const void* verts, size_t n_verts, const void* tris, const void* tri_mrgb, size_t n_tris,
                        const void* pos, const void* mrgb, size_t cap);

// The setup pass with its scratch and its three refusals (a bad index, a vertex that is not finite, a vertex out of range).
struct MeshFront {
    ScratchBuffer tq, off, tpart, bounds;
    MeshSummary ms;
    uint64_t columns = 0;
};
int voxelize_front(const char* who, const void* verts, size_t n_verts, const void* tris, size_t n_tris, hipStream_t stream, MeshFront* f);

// The least depth whose cube [-2^depth, 2^depth)^3 holds the candidate cells of all triangles (rule 5): at most 15.
uint32_t voxelize_depth(const MeshSummary& ms);

// The way out: m unique keys at `depth` and their leaf words -> *n and, with pos, the caller's arrays by the cap rule (decoded in
// place, or through staging buffers where pos or mrgb is not aligned for the kernel's stores).  Waits for the stream.
int voxelize_output(const char* who, const uint64_t* keys, const int32_t* words, size_t m, uint32_t depth, void* pos, void* mrgb, size_t cap,
                    hipStream_t stream, size_t* n);

}  // namespace vxrt
