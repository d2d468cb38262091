// morph_rule.h — the arithmetic of include/vxrt_morph.h as the kernels run it (morph.hip) and as a host compiler reads it
// (tests/test_morph_cpu.py builds a program of its own around this file): the 26-row offset table, the neighbour of a depth-15 path
// key under a row (stepped in the interleaved bits, with the range test), the two lookups of a key (in a block's tile, in the whole
// array), and what a neighbour mask means to each op.  Nothing from HIP is included, and the marker below is empty for a compiler
// that is not hipcc.  DESIGN.md §25.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VXRT_MORPH_FN __host__ __device__ inline
#else
#define VXRT_MORPH_FN inline
#endif

namespace vxrt {

// vxrt_morph_op
constexpr uint32_t kMorphDilate = 0, kMorphErode = 1, kMorphSurface = 2, kMorphMargin = 3;
constexpr uint32_t kMorphMaxSteps = 64;

// A block's tile and a thread's items: kMorphSpan consecutive keys per block, kMorphItems per thread.
constexpr uint32_t kMorphThreads = 256;
constexpr uint32_t kMorphItems = 8;
constexpr uint32_t kMorphSpan = kMorphThreads * kMorphItems;      // 2 048 = 2^kMorphTileSteps
constexpr uint32_t kMorphTileSteps = 11;
// What pads a tile behind its last key: greater than every key (48 bits).
constexpr uint64_t kMorphNoKey = ~uint64_t(0);

// Rule 2: first the 6 offsets with one nonzero axis, then the 12 with two, then the 8 with three; within a class ascending by
// 9 (dx + 1) + 3 (dy + 1) + (dz + 1).  Connectivity c uses rows 0 .. c - 1.
constexpr uint32_t kMorphRows = 26;
struct MorphOffset {
    int8_t d[3];
};
constexpr MorphOffset kMorphOffsets[kMorphRows] = {
    {{-1, 0, 0}},  {{0, -1, 0}},  {{0, 0, -1}},  {{0, 0, 1}},    {{0, 1, 0}},   {{1, 0, 0}},
    {{-1, -1, 0}}, {{-1, 0, -1}}, {{-1, 0, 1}},  {{-1, 1, 0}},   {{0, -1, -1}}, {{0, -1, 1}},
    {{0, 1, -1}},  {{0, 1, 1}},   {{1, -1, 0}},  {{1, 0, -1}},   {{1, 0, 1}},   {{1, 1, 0}},
    {{-1, -1, -1}}, {{-1, -1, 1}}, {{-1, 1, -1}}, {{-1, 1, 1}},  {{1, -1, -1}}, {{1, -1, 1}},
    {{1, 1, -1}},  {{1, 1, 1}}};

// The row of the negated offset: negation maps code s to 26 - s, so it reverses the order inside each class.
VXRT_MORPH_FN uint32_t opposite_row(uint32_t row) { return row < 6u ? 5u - row : row < 18u ? 23u - row : 43u - row; }

// The bits of connectivity c's rows.
VXRT_MORPH_FN uint32_t rows_of(uint32_t c) { return (uint32_t(1) << c) - 1u; }

// A path key at depth 15 holds u = p + 32768 per axis, bit k of u at bit 3k + 2 (x), 3k + 1 (y), 3k (z): 48 bits.
constexpr uint64_t kMorphAxisZ = 0x249249249249ull;      // the 16 bits of z; y's are << 1, x's << 2

// One axis's bits stepped by d in {-1, 0, 1}: + 1 carries through the other axes' bits once they are set (fill), - 1 borrows through
// them as they stand (they are zero in `part`), 0 adds nothing.  *ok = false where the coordinate would leave [0, 65535] (part is
// all ones and steps up, or zero and steps down): no wrap.  What depends on d alone is uniform over a kernel's grid.
VXRT_MORPH_FN uint64_t step_axis(uint64_t part, uint64_t mask, int d, bool* ok) {
    const uint64_t low = mask & (~mask + 1u);
    const uint64_t fill = d > 0 ? ~mask : 0u, add = d > 0 ? low : d < 0 ? ~low + 1u : 0u;
    const uint64_t edge = d > 0 ? mask : d < 0 ? 0u : ~uint64_t(0);      // no part is all 64 ones
    *ok = part != edge;
    return ((part | fill) + add) & mask;
}

// The key of the cell at row `row` from the cell of `key`; *ok = false where that cell lies outside the int16 range (the value
// returned is then some key of the range: it may be looked up, and the answer is dropped).
VXRT_MORPH_FN uint64_t neighbour_key(uint64_t key, uint32_t row, bool* ok) {
    const MorphOffset o = kMorphOffsets[row];
    bool okx, oky, okz;
    const uint64_t x = step_axis(key & (kMorphAxisZ << 2), kMorphAxisZ << 2, o.d[0], &okx);
    const uint64_t y = step_axis(key & (kMorphAxisZ << 1), kMorphAxisZ << 1, o.d[1], &oky);
    const uint64_t z = step_axis(key & kMorphAxisZ, kMorphAxisZ, o.d[2], &okz);
    *ok = okx && oky && okz;
    return x | y | z;
}

// A load from a "safe index": at where the array has it, else its last entry (entry 0 of an empty array's allocation, which is
// readable), for loads that are issued whether or not their value is used.
VXRT_MORPH_FN uint32_t morph_safe_index(uint32_t at, uint32_t count) {
    const uint32_t last = count ? count - 1u : 0u;
    return at < last ? at : last;
}

// The same for a 64-bit index, which the last block of a count near 2^32 needs: i clamped into an array of `count` entries.
VXRT_MORPH_FN uint32_t at_of(uint64_t i, uint32_t count) { return morph_safe_index(i < count ? uint32_t(i) : count, count); }

// The run heads of `count` sorted keys (run_heads.hip): entry i is one where it is the first, or differs above `shift` from the
// entry before.  cur and before are loaded from at_of(i) and at_of(i - 1): at i == 0 the latter wraps, is
// clamped, and its value is not used.
VXRT_MORPH_FN bool run_is_head(uint64_t cur, uint64_t before, uint64_t i, uint32_t count, uint32_t shift) {
    return i < count && (i == 0u || cur >> shift != before >> shift);
}

// Both lookups walk to the greatest index whose key is <= q, down from the top bit: with the walk at `at` and a step of `step`
// (a power of two), the key at walk_probe is loaded, whatever q is, and walk_take moves on to it or stays.  The kernel loads the
// probes of its kMorphItems walks side by side and takes them behind one wait.  `there`: the probe's index is inside the array.
VXRT_MORPH_FN uint64_t walk_probe(uint32_t at, uint64_t step) { return uint64_t(at) + step; }
VXRT_MORPH_FN uint32_t walk_take(uint64_t probed, uint64_t q, uint32_t at, uint64_t step, bool there) {
    return (there & (probed <= q)) ? uint32_t(walk_probe(at, step)) : at;
}

// Is q in the tile?  tile[0 .. kMorphSpan): a block's keys ascending, kMorphNoKey behind the last.  kMorphTileSteps probes at
// indices below kMorphSpan and one load more; with tile[0] > q the walk stays at 0 and the last test says no.
VXRT_MORPH_FN bool tile_has(const uint64_t* tile, uint64_t q) {
    uint32_t at = 0;
    for (uint32_t step = kMorphSpan >> 1; step != 0u; step >>= 1) at = walk_take(tile[walk_probe(at, step)], q, at, step, true);
    return tile[at] == q;
}

// The steps list_has needs for m keys: the bits of m - 1, at most 32.
VXRT_MORPH_FN uint32_t list_steps(uint32_t m) {
    uint32_t bits = 0;
    while (bits < 32u && (uint64_t(1) << bits) < uint64_t(m)) bits++;
    return bits;
}

// Is q among keys[0 .. m) (ascending, unique; readable at [0] even when m == 0)?  The same walk over the whole array, steps
// 2^(s - 1) for s = list_steps(m) down to 1: every load is unconditional from list_index, which clamps the probe into the array.
// A lane with active == false loads all the same and answers no: the kernel walks with every lane of a wave once one of them asks.
VXRT_MORPH_FN bool list_there(uint64_t probe, uint32_t m) { return probe < uint64_t(m); }
VXRT_MORPH_FN uint32_t list_index(uint64_t probe, uint32_t m) { return morph_safe_index(list_there(probe, m) ? uint32_t(probe) : m, m); }
VXRT_MORPH_FN bool list_has(const uint64_t* keys, uint32_t m, uint32_t steps, uint64_t q, bool active) {
    uint32_t at = 0;
    for (uint32_t s = steps; s != 0u; s--) {
        const uint64_t step = uint64_t(1) << (s - 1u), probe = walk_probe(at, step);
        at = walk_take(keys[list_index(probe, m)], q, at, step, active & list_there(probe, m));
    }
    return active & (m != 0u) & (keys[list_index(at, m)] == q);
}

// Where a neighbour q of a block's voxel is looked up: between the tile's first and last key the tile decides; outside them the
// whole array is asked.
VXRT_MORPH_FN bool tile_decides(uint64_t q, uint64_t first, uint64_t last) { return q >= first && q <= last; }

// ERODE keeps a cell whose c neighbours are all present (mask: bit r = the cell at row r is in the set).  A neighbour outside the
// range is never present, so a cell on the range's edge goes.
VXRT_MORPH_FN bool keep_eroded(uint32_t mask, uint32_t c) { return (mask & rows_of(c)) == rows_of(c); }

// DILATE: the least row of the first c whose cell is in the set (a new cell's mask is never empty); kMorphRows when there is none.
VXRT_MORPH_FN uint32_t first_source(uint32_t mask, uint32_t c) {
    const uint32_t m = mask & rows_of(c);
    uint32_t row = 0;
    while (row < kMorphRows && (m >> row & 1u) == 0u) row++;
    return row;
}

// DILATE: the rows (of the first c) at which a voxel of the set offers itself as a source: the neighbour is in range and absent.
VXRT_MORPH_FN uint32_t offer_rows(uint64_t key, uint32_t mask, uint32_t c) {
    uint32_t rows = 0;
    for (uint32_t r = 0; r < kMorphRows; r++) {
        bool ok;
        (void)neighbour_key(key, r, &ok);
        rows |= (ok ? 1u : 0u) << r;
    }
    return rows & ~mask & rows_of(c);
}

// An offer as it is sorted: the new cell's key above the row at which that cell sees the source (the opposite row), so that the
// first entry of a cell after the sort is its first_source.
constexpr uint32_t kMorphOfferShift = 5;
VXRT_MORPH_FN uint64_t offer_key(uint64_t cell, uint32_t row_from_source) { return cell << kMorphOfferShift | uint64_t(opposite_row(row_from_source)); }
VXRT_MORPH_FN uint64_t offer_cell(uint64_t offer) { return offer >> kMorphOfferShift; }

}  // namespace vxrt
