// setops.h — what api_setops.hip (host side of vxrt_setops.h) and setops.hip (its kernel) share.  DESIGN.md §24.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "setops_rule.h"

namespace vxrt {

// The merge runs blocks of kSetopThreads threads over kSetopSpan consecutive items of the merged sequence each, kSetopItems per
// thread (setops_rule.h), so a grid has setop_blocks(ma + mb) <= 2^21 blocks for fewer than 2^32 items.
inline uint32_t setop_blocks(uint64_t items) { return uint32_t((items + kSetopSpan - 1) / kSetopSpan); }

struct SetopArgs {
    const uint64_t* keys_a;     // ma unique path keys at depth 15, ascending; readable at [0] even when ma == 0
    const uint32_t* words_a;    // their leaf words (readable at [0] even when ma == 0), or nullptr: lists without mrgb
    const uint64_t* keys_b;     // mb keys, as keys_a
    const uint32_t* words_b;    // their leaf words, or nullptr (no mrgb, or b is a mask: INTERSECT, DIFFERENCE)
    uint32_t ma, mb;            // 0 < ma + mb < 2^32
    uint32_t op;                // vxrt_list_op; kListChanged needs both words
    uint64_t* part;             // setop_blocks(ma + mb) entries: written with the blocks' counts (counting), read as their offsets (emitting)
    uint64_t* out_keys;         // emitting: the kept keys at the scanned offsets, ascending and unique; nullptr: counting
    uint32_t* out_words;        // ... and the leaf word of each from its own side; nullptr for lists without mrgb
};

// Counting (a.out_keys == nullptr): part[b] = the items of block b that the op keeps.  Emitting: those items' keys and words at
// part[b] onward in merged order, which is ascending path order.
hipError_t launch_setop_merge(const SetopArgs& a, hipStream_t s);

}  // namespace vxrt
