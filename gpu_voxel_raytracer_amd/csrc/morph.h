// morph.h — what api_morph.hip (host side of vxrt_morph.h) and morph.hip (its kernels) share.  DESIGN.md §25.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "morph_rule.h"

namespace vxrt {

// Every kernel here runs blocks of kMorphThreads threads over kMorphSpan consecutive entries each, kMorphItems per thread
// (morph_rule.h), so a grid has morph_blocks(count) <= 2^21 blocks for fewer than 2^32 entries.
inline uint32_t morph_blocks(uint64_t count) { return uint32_t((count + kMorphSpan - 1) / kMorphSpan); }

// The set a step works on: m > 0 unique path keys at depth 15, ascending, and their leaf words (nullptr: positions only).
struct MorphSet {
    const uint64_t* keys;
    const uint32_t* words;
    uint32_t m;
};

// masks[i] = bit r set where the cell at row r < c from keys[i] is in the set; part[b] = what block b's voxels give the step:
// op == kMorphErode the voxels keep_eroded keeps, op == kMorphDilate the offers they make (offer_rows).  part: morph_blocks(m)
// entries.  tile == false sends every lookup to the whole array: the product's route, which measured faster than the tile
// (DESIGN.md §25); tile == true is kept for scripts/morph_latency.py to measure against.
hipError_t launch_morph_mask(const MorphSet& s, uint32_t c, uint32_t op, bool tile, uint32_t* masks, uint64_t* part, hipStream_t stream);

// ERODE's write: the voxels keep_eroded keeps, at part[b] onward (part scanned), ascending as they stood.
hipError_t launch_morph_keep(const MorphSet& s, uint32_t c, const uint32_t* masks, const uint64_t* part, uint64_t* out_keys,
                             uint32_t* out_words, hipStream_t stream);

// DILATE's write: every offer (offer_key of the neighbour and the row, the source's leaf word) at part[b] onward, in no order
// the caller may rely on but the same one every time.
hipError_t launch_morph_offer(const MorphSet& s, uint32_t c, const uint32_t* masks, const uint64_t* part, uint64_t* out_offers,
                              uint32_t* out_words, hipStream_t stream);

// The first offer of each cell of `count` sorted offers.  Counting (out_keys == nullptr): part[b] = the cells that begin in block
// b, morph_blocks(count) entries.  Emitting: their keys (offer_cell) and words at part[b] onward, ascending and unique.
hipError_t launch_morph_first(const uint64_t* offers, const uint32_t* words, uint32_t count, uint64_t* part, uint64_t* out_keys,
                              uint32_t* out_words, hipStream_t stream);

}  // namespace vxrt
