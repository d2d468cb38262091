// shape.h — what api_shape.hip (host side of vxrt_shape.h) and shape.hip (its kernels) share.  DESIGN.md §29.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vxrt {

// A tile is an aligned 16^3 cube of cells, aligned in u = cell + 32768: the cells that share a path key's upper 36 bits.  One block
// of kShapeThreads threads takes one tile, kShapeItems cells per thread: thread t's cells have the path indices 16 t .. 16 t + 15
// within the tile, so thread order is path order.
constexpr uint32_t kShapeThreads = 256;
constexpr uint32_t kShapeItems = 16;
constexpr uint32_t kShapeTileBits = 36;                      // path_key15 >> 12
constexpr uint64_t kShapeTileMask = (uint64_t(1) << kShapeTileBits) - 1;
// what the counting pass found out about a tile, kept in its key's top bits for the emitting pass
constexpr uint32_t kShapeClassShift = 62;
constexpr uint64_t kShapeMixed = 0, kShapeOutside = 1, kShapeWhole = 2;

struct ShapeArgs {
    int32_t m[3][3];        // vxrt_affine
    int64_t t[3];
    uint32_t kind;          // vxrt_shape_kind
    int64_t r2;             // 2 r
    int64_t h2[3];          // 2 h[i]
    int64_t reach[3];       // no cell with |P_i| > reach[i] is inside: the shape's bounding box in shape space
    int32_t lo[3], hi[3];   // the box, half-open, not empty
    uint32_t tlo[3];        // the least tile that meets the box per axis, as (lo + 32768) >> 4 ...
    uint32_t text[3];       // ... and how many tiles do
    uint32_t tiles;         // their product
    uint64_t* keys;         // tiles entries: the tiles' keys (path_key15 >> 12), ascending once sorted; the counting pass adds the class
    uint64_t* part;         // tiles + 1 entries: written with the tiles' counts (counting), read as their offsets (emitting)
    uint8_t* out_pos;       // emitting: 6 bytes per voxel at the scanned offsets; nullptr: counting
    uint8_t* out_mrgb;      // 4 bytes per voxel, or nullptr
    uint32_t word;          // (mrgb[0] & 0x7f) << 24 | r << 16 | g << 8 | b
#ifdef VXRT_SHAPE_SORTED
    uint32_t cells;         // the box's cells, < 2^32; cell c is lo + (c / (ext[1] ext[2]), c / ext[2] % ext[1], c % ext[2])
    uint32_t ext[3];
    uint64_t* out_keys;     // emitting: the voxels' path keys at the scanned offsets, thread by thread; nullptr: counting
#endif
};

// keys[i] = the key of the i-th tile that meets the box, in x-major order of the tile grid: not path order; the caller sorts.
hipError_t launch_shape_tiles(const ShapeArgs& a, hipStream_t s);

// Counting (a.out_pos == nullptr): part[b] = the cells of tile keys[b] that are in the box and inside the shape, and the tile's class
// into keys[b].  Emitting: those cells' positions and bytes at part[b] onward in path order, by byte stores: any alignment.
hipError_t launch_shape(const ShapeArgs& a, hipStream_t s);

#ifdef VXRT_SHAPE_SORTED
// -DVXRT_SHAPE_SORTED (an A/B build, scripts/ab_build.sh): the route the tile order is measured against, in the
// transform's shape.  Blocks of kShapeThreads threads over kShapeSpan consecutive cells of the box, 8 per thread (thread t's cells
// t, t + 256, ...): part[b] = the block's cells inside the shape (counting), or their path keys at part[b] onward in thread order
// (emitting): not path order; the caller sorts the keys and decodes them.
constexpr uint32_t kShapeSpan = kShapeThreads * 8;
inline uint32_t shape_blocks(uint64_t cells) { return uint32_t((cells + kShapeSpan - 1) / kShapeSpan); }
hipError_t launch_shape_linear(const ShapeArgs& a, hipStream_t s);
// keys[0 .. n) -> pos (3 int16 each) and, unless nullptr, mrgb (the bytes of `word` each) by byte stores
hipError_t launch_shape_decode(const uint64_t* keys, uint32_t n, uint32_t word, uint8_t* pos, uint8_t* mrgb, hipStream_t s);
#endif

}  // namespace vxrt
