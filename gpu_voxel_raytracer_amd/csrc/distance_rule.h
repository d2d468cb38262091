// distance_rule.h — the arithmetic of include/vxrt_distance.h as the kernels run it (distance.hip) and as a host compiler reads it
// (tests/test_distance_cpu.py builds a program of its own around this file): the rank of an offset, the radius of a squared radius,
// the nearest set bit of an occupancy row, the two bounded-minimum steps with their tie-breaks, a tile's 12-bit path index to
// (x, y, z) and back, and a tile key's neighbour with its range test.  Nothing from HIP and nothing of the project's is included,
// and the marker below is empty for a compiler that is not hipcc.  DESIGN.md §30.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VXRT_DISTANCE_FN __host__ __device__ inline
#else
#define VXRT_DISTANCE_FN inline
#endif

namespace vxrt {

// vxrt_distance_mode
constexpr uint32_t kDistanceDepth = 0, kDistanceField = 1, kDistanceErode = 2, kDistanceDilate = 3;
constexpr uint32_t kDistanceFar = 0xFFFFu;        // no cell within max_d2; also "no value" between the passes
constexpr uint32_t kDistanceMaxD2 = 256;
constexpr uint32_t kDistanceMaxR = 16;            // R * R <= kDistanceMaxD2

// A block takes one tile of 16^3 cells, 16 path indices per thread; its window is the tile and R cells around it.
constexpr uint32_t kDistanceThreads = 256;
constexpr uint32_t kDistanceItems = 16;
constexpr uint32_t kDistanceTile = 16;
constexpr uint32_t kDistanceMaxWindow = kDistanceTile + 2 * kDistanceMaxR;      // 48: a row of the window fits a 64-bit word
constexpr uint32_t kDistanceRows = kDistanceMaxWindow * kDistanceMaxWindow;     // the (y, z) rows of the window, at most
constexpr uint32_t kDistancePlane = kDistanceTile * kDistanceMaxWindow;         // pass 1's plane: 16 x by at most 48 y
constexpr uint32_t kDistanceSlab = kDistanceTile * kDistanceTile * kDistanceMaxWindow;      // pass 2's result: 16 x by 16 y by at most 48 z
constexpr uint32_t kDistanceWindowTiles = 27;
constexpr int kDistanceNoStep = 127;              // pass 1: the row has no set bit within R

// Rule 5: rank(0) = 0, rank(-k) = 2k - 1, rank(+k) = 2k.
VXRT_DISTANCE_FN uint32_t distance_rank(int d) { return d == 0 ? 0u : d < 0 ? uint32_t(-2 * d - 1) : uint32_t(2 * d); }
// ... and the offset of a rank: 0, -1, +1, -2, +2, ...  A pass that visits ranks 0 .. 2 R in order and keeps a strictly smaller
// value breaks ties by rank.
VXRT_DISTANCE_FN int distance_offset(uint32_t rank) { return (rank & 1u) ? -int((rank + 1u) >> 1) : int(rank >> 1); }

// Rule 2: the largest R with R * R <= max_d2 (max_d2 in 1 .. 256: R in 1 .. 16).
VXRT_DISTANCE_FN uint32_t distance_radius(uint32_t max_d2) {
    uint32_t r = 0;
    while (r < kDistanceMaxR && (r + 1u) * (r + 1u) <= max_d2) r++;
    return r;
}

// Pass 1: the offset dx, |dx| <= r, of the set bit of `row` nearest to bit c (c < 64), the lower bit at equal distance (rank's
// order); kDistanceNoStep where there is none.  Bit c itself gives 0.
VXRT_DISTANCE_FN int distance_nearest(uint64_t row, uint32_t c, uint32_t r) {
    const uint64_t upto = c >= 63u ? ~uint64_t(0) : (uint64_t(2) << c) - 1u;      // bits 0 .. c
    const uint64_t below = row & upto, above = row & ~upto;
    uint32_t down = 64u, up = 64u;                                                // distances; 64: none
    if (below != 0u) down = c - (63u - uint32_t(__builtin_clzll(below)));
    if (above != 0u) up = uint32_t(__builtin_ctzll(above)) - c;
    if (down <= up) return down <= r ? -int(down) : kDistanceNoStep;
    return up <= r ? int(up) : kDistanceNoStep;
}

// Pass 2's step: the row at offset dy from the cell's has its nearest bit at dx (or kDistanceNoStep).  Called with dy in rank
// order; a strictly smaller dx^2 + dy^2 takes over.
VXRT_DISTANCE_FN void distance_take_row(int dx, int dy, uint32_t* best, int* best_dy) {
    const uint32_t d2 = uint32_t(dx * dx + dy * dy);
    if (dx != kDistanceNoStep && d2 < *best) {
        *best = d2;
        *best_dy = dy;
    }
}

// Pass 3's step: the plane at offset dz has d2xy (or kDistanceFar) for the cell's column.  Called with dz in rank order.
VXRT_DISTANCE_FN void distance_take_plane(uint32_t d2xy, int dz, uint32_t* best, int* best_dz) {
    const uint32_t d2 = d2xy + uint32_t(dz * dz);
    if (d2xy != kDistanceFar && d2 < *best) {
        *best = d2;
        *best_dz = dz;
    }
}

// Rule 6: is the tile's cell in the result?  in_set: the cell is a voxel of S; d2: the squared distance the passes found (to the
// nearest empty cell for DEPTH and ERODE, to the nearest voxel for FIELD and DILATE; kDistanceFar where none is within R per axis).
VXRT_DISTANCE_FN bool distance_emits(uint32_t mode, bool in_set, uint32_t d2, uint32_t max_d2) {
    const bool near = d2 <= max_d2;
    return mode == kDistanceDepth ? in_set : mode == kDistanceErode ? in_set && !near : mode == kDistanceField ? !in_set && near : near;
}
// ... and the d2 it carries.
VXRT_DISTANCE_FN uint32_t distance_value(uint32_t d2, uint32_t max_d2) { return d2 <= max_d2 ? d2 : kDistanceFar; }

// A tile's cells in path order: bit k of x, y, z at bits 3k + 2, 3k + 1, 3k of the 12-bit index.
VXRT_DISTANCE_FN uint32_t distance_compact4(uint32_t v) {
    return (v & 1u) | (v >> 2 & 2u) | (v >> 4 & 4u) | (v >> 6 & 8u);
}
VXRT_DISTANCE_FN uint32_t distance_spread4(uint32_t v) {
    return (v & 1u) | (v & 2u) << 2 | (v & 4u) << 4 | (v & 8u) << 6;
}
VXRT_DISTANCE_FN void distance_cell_of(uint32_t index, uint32_t* x, uint32_t* y, uint32_t* z) {
    *x = distance_compact4(index >> 2);
    *y = distance_compact4(index >> 1);
    *z = distance_compact4(index);
}
VXRT_DISTANCE_FN uint32_t distance_index_of(uint32_t x, uint32_t y, uint32_t z) {
    return distance_spread4(x) << 2 | distance_spread4(y) << 1 | distance_spread4(z);
}

// A tile key is a path key at depth 15 without its low 12 bits: 36 bits, bit k of the tile's coordinate (0 .. 4095 per axis) at
// bits 3k + 2 (x), 3k + 1 (y), 3k (z).
VXRT_DISTANCE_FN uint32_t distance_compact12(uint64_t v) {
    uint32_t out = 0;
    for (uint32_t k = 0; k < 12u; k++) out |= uint32_t(v >> (3u * k) & 1u) << k;
    return out;
}
VXRT_DISTANCE_FN uint64_t distance_spread12(uint32_t v) {
    uint64_t out = 0;
    for (uint32_t k = 0; k < 12u; k++) out |= uint64_t(v >> k & 1u) << (3u * k);
    return out;
}
// The tile at (dx, dy, dz) tiles from `tile`, each in {-1, 0, 1}; *ok = false where it lies outside the int16 range (rule 3: the
// value returned is then `tile` itself).
VXRT_DISTANCE_FN uint64_t distance_tile_step(uint64_t tile, int dx, int dy, int dz, bool* ok) {
    const int x = int(distance_compact12(tile >> 2)) + dx, y = int(distance_compact12(tile >> 1)) + dy, z = int(distance_compact12(tile)) + dz;
    *ok = x >= 0 && x < 4096 && y >= 0 && y < 4096 && z >= 0 && z < 4096;
    if (!*ok) return tile;
    return distance_spread12(uint32_t(x)) << 2 | distance_spread12(uint32_t(y)) << 1 | distance_spread12(uint32_t(z));
}
// Tile `i` (0 .. 26) of a window is the one at (i / 9 - 1, i / 3 % 3 - 1, i % 3 - 1) tiles from its centre.
VXRT_DISTANCE_FN uint64_t distance_window_tile(uint64_t tile, uint32_t i, bool* ok) {
    return distance_tile_step(tile, int(i / 9u) - 1, int(i / 3u % 3u) - 1, int(i % 3u) - 1, ok);
}

// The walk to the greatest index of keys[lo .. hi) whose key is <= q, by `steps` probes of 2^(steps - 1) .. 1 cells: every probe is
// loaded, clamped into [0, last], whatever q is.  With keys[lo] > q (or lo == hi) the walk stays at lo.  2^steps >= hi - lo.
VXRT_DISTANCE_FN uint32_t distance_walk(const uint64_t* keys, uint32_t last, uint32_t lo, uint32_t hi, uint32_t steps, uint64_t q) {
    uint32_t at = lo;
    for (uint32_t s = steps; s != 0u; s--) {
        const uint64_t probe = uint64_t(at) + (uint64_t(1) << (s - 1u));
        const uint64_t k = keys[probe < uint64_t(last) ? uint32_t(probe) : last];
        if (probe < uint64_t(hi) && k <= q) at = uint32_t(probe);
    }
    return at;
}
// The first index of keys[0 .. m) (ascending, m > 0) whose key is >= q; m where there is none.
VXRT_DISTANCE_FN uint32_t distance_lower_bound(const uint64_t* keys, uint32_t m, uint32_t steps, uint64_t q) {
    if (q == 0u) return 0u;
    const uint32_t at = distance_walk(keys, m - 1u, 0u, m, steps, q - 1u);      // the greatest index with key < q, or 0
    return keys[at] < q ? at + 1u : 0u;
}
// The probes a walk over m entries needs: the bits of m, at most 32.
VXRT_DISTANCE_FN uint32_t distance_steps(uint32_t m) {
    uint32_t bits = 0;
    while (bits < 32u && (uint64_t(1) << bits) <= uint64_t(m)) bits++;
    return bits;
}

}  // namespace vxrt
