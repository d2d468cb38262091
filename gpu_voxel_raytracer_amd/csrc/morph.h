// morph.h — what api_morph.hip (host side of vxrt_morph.h) and morph.hip (its kernels) share, and the block geometry that
// run_heads.hip and mesh.hip run too.  DESIGN.md §25.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "morph_rule.h"

namespace vxrt {

// Every kernel here runs blocks of kMorphThreads threads over kMorphSpan consecutive entries each, kMorphItems per thread
// (morph_rule.h), so a grid has morph_blocks(count) <= 2^21 blocks for fewer than 2^32 entries.
inline uint32_t morph_blocks(uint64_t count) { return uint32_t((count + kMorphSpan - 1) / kMorphSpan); }

// A thread's item k.  The counting and compacting kernels take a thread's items side by side (entry base + 8 t + k), so that a
// block's output is in the order of its input; the others take them a block's width apart (entry base + 256 k + t), so that a
// wave's loads and stores are neighbours.  An entry's index is 64 bits wide: the last block of a count near 2^32 reaches past it;
// at_of (morph_rule.h) clamps it into its array.
__device__ __forceinline__ uint64_t item_beside(uint32_t k) { return uint64_t(blockIdx.x) * kMorphSpan + threadIdx.x * kMorphItems + k; }
__device__ __forceinline__ uint64_t item_apart(uint32_t k) { return uint64_t(blockIdx.x) * kMorphSpan + k * kMorphThreads + threadIdx.x; }

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
// the caller may rely on but the same one every time.  Sorted, the first offer of each cell is a run head above kMorphOfferShift
// (run_heads.h), and its key there is the cell's (offer_cell).
hipError_t launch_morph_offer(const MorphSet& s, uint32_t c, const uint32_t* masks, const uint64_t* part, uint64_t* out_offers,
                              uint32_t* out_words, hipStream_t stream);

}  // namespace vxrt
