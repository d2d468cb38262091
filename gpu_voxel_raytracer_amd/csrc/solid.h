// solid.h — what api_solid.hip (host side of vxrt_solid.h) and solid.hip (its kernels) share.  DESIGN.md §18.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "voxelize.h"

namespace vxrt {

// A work item of the crossing passes is one (triangle, z-column) pair: the columns (x, y) whose centre lies inside the triangle's
// snapped bounds on x and y (rule 1; a triangle may have none).  Items are numbered in triangle order, then y, then x; a crossing's
// position is a prefix sum over that numbering, an interior cell's a prefix sum over the sorted pairs of crossings.
//
// A crossing's sort key, relative to the least candidate cell of the mesh per axis (MeshSummary::lo) so that it takes as few radix
// passes as the mesh's extent allows: (x - lo_x) << (by + bz) | (y - lo_y) << bz | (k - lo_z).
struct SolidKeying {
    int32_t lo[3];
    uint32_t by, bz;      // the bits of the y and the k field
    uint32_t bits;        // bx + by + bz <= 49
};
SolidKeying solid_keying(const MeshSummary& ms);

// The first odd column of a mesh that is not closed: its cell and how many crossings it has.
struct SolidOpen {
    int32_t x, y;
    uint32_t crossings, pad;
};

// tq: voxelize_setup's snapped triangles (n_tris > 0).  zoff[t] = the z-columns of the triangles before t, zoff[n_tris] = *columns.
// part: vox_blocks(n_tris) + 1 words.  Waits for the result.
int solid_columns(const VoxTri* tq, uint32_t n_tris, uint64_t* zoff, uint64_t* part, hipStream_t stream, uint64_t* columns);

// The crossing pass over the columns items (0 < columns < 2^32), counting: part[b] = the crossings of items [256 b, 256 b + 256)
// scanned exclusively, part[vox_blocks(columns)] = *crossings.  Waits for the result.
int solid_count(const VoxTri* tq, const uint64_t* zoff, uint32_t n_tris, uint32_t columns, uint64_t* part, hipStream_t stream,
                uint64_t* crossings);

// The same pass, writing crossing h's key to keys[h], h in item order.  part: as solid_count left it.
hipError_t solid_emit(const VoxTri* tq, const uint64_t* zoff, uint32_t n_tris, uint32_t columns, const uint64_t* part, SolidKeying keying,
                      uint64_t* keys, hipStream_t stream);

// keys: the crossings ascending (0 < crossings < 2^32).  Pair j is keys[2j], keys[2j + 1]; loff[j] = the interior cells of the pairs
// before j, loff[crossings / 2] = *cells (loff holds crossings / 2 + 1 words, part vox_blocks(crossings / 2) + 1).  *closed is
// false when the count is odd or a pair spans two columns; *open then names the first odd column and nothing else is meaningful.
// Waits for the result.  who: the API call, for the two small allocations this makes (VXRT_E_DEVICE when one fails).
int solid_pairs(const uint64_t* keys, uint32_t crossings, SolidKeying keying, uint64_t* loff, uint64_t* part, const char* who,
                hipStream_t stream, bool* closed, SolidOpen* open, uint64_t* cells);

// Interior cell i (of cells, 0 < cells < 2^32) -> its path key at `depth` in out_keys[i] and, with out_vals, `word` in out_vals[i].
hipError_t solid_fill(const uint64_t* keys, const uint64_t* loff, uint32_t pairs, uint32_t cells, SolidKeying keying, uint32_t depth,
                      uint32_t word, uint64_t* out_keys, uint32_t* out_vals, hipStream_t stream);

}  // namespace vxrt
