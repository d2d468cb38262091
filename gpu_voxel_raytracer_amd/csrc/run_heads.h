// run_heads.h — the run heads of a sorted key array, counted per block and written in order (run_heads.hip): what api_morph.hip
// (the first offer of each cell, shift 5) and api_mesh.hip (the distinct corners, shift 0) ask of their sorted keys.  The host half
// is list_ops.h's run_heads_count / run_heads_emit.  DESIGN.md §26.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vxrt {

// Entry i of keys[0 .. n), n > 0, is a head where run_is_head says so (morph_rule.h).  morph.h's geometry: morph_blocks(n) blocks.
// Counting (out_keys == nullptr): part[b] = the heads in block b.  Emitting (part scanned): head number h writes keys[i] >> shift
// to out_keys[h] and, where words and out_words are both given, words[i] to out_words[h].
hipError_t launch_run_heads(const uint64_t* keys, const uint32_t* words, uint32_t n, uint32_t shift, uint64_t* part, uint64_t* out_keys,
                            uint32_t* out_words, hipStream_t stream);

}  // namespace vxrt
