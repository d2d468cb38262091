// list_ops.h — the host pipeline behind the operators on voxel lists in device memory (api_transform.hip, api_setops.hip,
// api_morph.hip, api_mesh.hip, api_shape.hip, api_distance.hip): a list keyed at depth 15, sorted and deduplicated; a counting
// kernel's partials and their scan's total read back; the run heads of sorted keys, counted and written; two sorted unique sets
// merged under a set operation; the bits a sort of tile keys has to look at; the checks of the two output arrays and the decode
// into them.  The double-buffered sort itself is device_build.h's KeySort.  Host code only: the kernels are device_edit.hip's,
// device_build.hip's, run_heads.hip's, setops.hip's and transform.hip's.  DESIGN.md §26.
#pragma once
#include <utility>

#include "ctx.h"
#include "device_build.h"
#include "edit.h"
#include "morph.h"
#include "setops.h"

namespace vxrt {

// A sorted unique set as the host passes it around is a MorphSet (morph.h): m unique ascending path keys at depth 15 and their leaf
// words, or nullptr for positions only.  Between operators m may be 0; keys (and words, where there are any) are readable all the same.

// launch_exclusive_scan over part[0 .. blocks), then part[blocks] (the total) -> the host.  Waits.
int scan_total(uint64_t* part, uint32_t blocks, hipStream_t s, uint64_t* total);
// part[0 .. blocks] for a counting kernel of morph.h's geometry over `count` entries and the scan behind it.
int alloc_part(ScratchBuffer* part, uint64_t count, const char* who);

// One list through the front: keyed by the device editor's pass, sorted, one entry per position with the last entry's bytes.
// with_vals == false leaves the leaf words behind (view.words == nullptr).  An empty list gets the 16 readable bytes of
// alloc_scratch per array, which the merge's clamped loads may touch and never use.
struct KeyedList {
    ListScratch ls;
    ScratchBuffer leaves;
    MorphSet view{nullptr, nullptr, 0u};
};
// bounds: where to put the list's bounding box (n > 0), or nullptr.  Waits for the count.
int key_list(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, bool with_vals, hipStream_t s, const char* who, KeyedList* out,
             ListBounds* bounds);

// A set in exactly sized buffers of its own.
struct OwnedSet {
    ScratchBuffer keys, words;
    MorphSet view{nullptr, nullptr, 0u};
    void take(OwnedSet* from) {      // what this held goes with `from`
        keys.swap(from->keys);
        words.swap(from->words);
        view = from->view;
    }
};
// whose: "a step's", "the result's": whose keys and leaf words a failed allocation names.
int alloc_set(OwnedSet* out, uint64_t count, bool with_vals, const char* who, const char* whose);

// The run heads of keys[0 .. n), 0 < n < 2^32, sorted (run_heads.h: entry 0 and every entry that differs from the one before
// above `shift`), in two phases.
struct RunHeads {
    const uint64_t* keys = nullptr;
    uint32_t n = 0, shift = 0;
    ScratchBuffer part;      // must outlive the emitting launch on the stream
    uint64_t count = 0;
};
// Launches the counting kernel and the scan -> rh->count.  Waits.
int run_heads_count(const uint64_t* keys, uint32_t n, uint32_t shift, hipStream_t s, const char* who, RunHeads* rh);
// The heads' keys >> shift -> out_keys[0 .. rh->count) and, where both are given, their entries of `words` -> out_words.  Does not wait.
int run_heads_emit(const RunHeads& rh, const uint32_t* words, uint64_t* out_keys, uint32_t* out_words, hipStream_t s);
// Both, into *out, exactly sized (with_words: `words` come along).  Does not wait after the emitting launch; rh->part goes with *rh.
int run_heads(const uint64_t* keys, const uint32_t* words, uint32_t n, uint32_t shift, bool with_words, hipStream_t s, const char* who,
              const char* whose, RunHeads* rh, OwnedSet* out);

// Morton keys of tiles whose coordinates lie in [first, last] per axis agree above these many bits: what a sort of them looks at.
uint32_t tile_sort_bits(const uint32_t first[3], const uint32_t last[3]);

// The merge of setops.hip over two sets, 0 < a.m + b.m < 2^32, in two phases.  b.words == nullptr beside a.words takes b as a mask.
struct SetMerge {
    SetopArgs args{};
    ScratchBuffer part;      // must outlive the emitting merge on the stream
    uint64_t count = 0;
};
// Launches the counting merge and the scan -> mg->count.  Waits.
int merge_count(const MorphSet& a, const MorphSet& b, uint32_t op, hipStream_t s, const char* who, SetMerge* mg);
// mg->count > 0: *out, exactly sized (with words where a has them), and the emitting merge into it.  Does not wait.
int merge_emit(SetMerge* mg, hipStream_t s, const char* who, const char* whose, OwnedSet* out);

// The output arrays of an operator.  The pairing rule, which looks at no memory: with bytes in the input, out_pos and out_mrgb come
// both or neither; without, out_mrgb is refused ("out_mrgb without <input>").
int check_output_pair(bool with_vals, const void* out_pos, const void* out_mrgb, const char* who, const char* input);
// ... and check_device_array on each that is given, at room for `cap` voxels; on an input list of n entries (none: not looked at).
int check_input_list(const vxrt_ctx* c, const void* pos, const void* mrgb, size_t n, const char* who, const char* pos_name, const char* mrgb_name);
int check_output_arrays(const vxrt_ctx* c, const void* out_pos, const void* out_mrgb, size_t cap, const char* who);

// The end of an operator whose result has `count` voxels: *n_out = count; more than `cap` of them into out_pos is refused ("N
// voxels, room for CAP").  A counting call (out_pos == nullptr) and an empty result then have nothing to write.
int list_room(uint64_t count, const void* out_pos, size_t cap, const char* who, size_t* n_out);
// transform.hip's decode of keys[0 .. count) and words into the caller's arrays.  Waits.
int decode_list(const uint64_t* keys, const uint32_t* words, uint64_t count, int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], hipStream_t s);

}  // namespace vxrt
