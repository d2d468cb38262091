// transform.h — what api_transform.hip (host side of vxrt_transform.h) and transform.hip (its kernels) share.  DESIGN.md §23.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace vxrt {

// The pull runs blocks of kPullThreads threads over kPullSpan consecutive destination cells each, kPullItems cells per thread (the
// layout of query.hip's lookup), so a grid has pull_blocks(cells) <= 2^21 blocks for a box below 2^32 cells.
constexpr uint32_t kPullThreads = 256;
constexpr uint32_t kPullItems = 8;
constexpr uint32_t kPullSpan = kPullThreads * kPullItems;
constexpr uint32_t kPullSample = 1024;   // keys a block stages in LDS (8 KB): the whole source list, or an evenly spaced sample of it

inline uint32_t pull_blocks(uint64_t cells) { return uint32_t((cells + kPullSpan - 1) / kPullSpan); }

struct PullArgs {
    int32_t m[3][3];        // vxrt_affine
    int64_t t[3];
    int32_t lo[3];          // the box's least corner
    uint32_t ext[3];        // its extent per axis, each > 0; cell c is lo + (c / (ext[1] ext[2]), c / ext[2] % ext[1], c % ext[2])
    uint32_t cells;         // their product, < 2^32
    const uint64_t* keys;   // the source: count > 0 unique path keys at depth 15, ascending
    const int32_t* words;   // their leaf words, or nullptr (a list without mrgb)
    uint32_t count;
    uint32_t steps;         // set by launch_transform_pull: the search steps in global memory behind the staged keys, 0 when the list fits
    int32_t src_lo[3], src_hi[3];   // the source's bounding box, inclusive
    uint64_t* part;         // pull_blocks(cells) entries: written with the blocks' counts (counting), read as their offsets (emitting)
    uint64_t* out_keys;     // emitting: (key of d, leaf word of s) at the scanned offsets; nullptr: counting
    uint32_t* out_words;    // nullptr for a list without mrgb
};

// Counting (a.out_keys == nullptr): part[b] = the cells of block b that pull a source voxel.  Emitting: those cells' keys and words at
// part[b] onward, thread by thread (thread t's cells t, t + 256, ... together, in that order): not cell order, not path order; the
// caller sorts.
hipError_t launch_transform_pull(const PullArgs& a, hipStream_t s);

// keys[0 .. n) (path keys at depth 15) and their leaf words (or nullptr) -> pos (3 int16 each) and mrgb (4 bytes each, or nullptr) by
// byte stores: any alignment.
hipError_t launch_transform_decode(const uint64_t* keys, const uint32_t* words, uint32_t n, uint8_t* pos, uint8_t* mrgb, hipStream_t s);

}  // namespace vxrt
