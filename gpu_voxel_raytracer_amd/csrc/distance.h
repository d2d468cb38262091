// distance.h — what api_distance.hip (host side of vxrt_distance.h) and distance.hip (its kernels) share.  DESIGN.md §30.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "distance_rule.h"

namespace vxrt {

// The run heads of a sorted array: entry i is a head where i == 0 or keys[i] >> shift differs from keys[i - 1] >> shift.  Blocks of
// kDistanceThreads entries, one per thread.
inline uint32_t distance_head_blocks(uint64_t n) { return uint32_t((n + kDistanceThreads - 1) / kDistanceThreads); }

// Counting (out == nullptr): part[b] = the heads in block b, distance_head_blocks(n) entries.  Emitting (part scanned): head number h
// writes keys[i] >> shift to out[h]; with spread, the 27 tiles of its window (distance_window_tile; a tile outside the range gives
// the head's own key once more) to out[27 h .. 27 h + 26]: not in order; the caller sorts and takes the heads again.
hipError_t launch_distance_heads(const uint64_t* keys, uint32_t n, uint32_t shift, bool spread, uint64_t* part, uint64_t* out, hipStream_t s);

struct DistanceArgs {
    const uint64_t* keys;      // the list: m > 0 unique ascending path keys at depth 15 ...
    const uint32_t* words;     // ... and their leaf words; nullptr: positions only (and every counting call)
    uint32_t m;
    uint32_t steps;            // distance_steps(m)
    const uint64_t* tiles;     // the candidate tiles' keys (path key >> 12), ascending and unique: one block each
    uint32_t ntiles;
    uint64_t* part;            // ntiles + 1 entries: written with the tiles' counts (counting), read as their offsets (emitting)
    uint32_t mode;             // vxrt_distance_mode
    uint32_t max_d2;           // 1 .. 256
    uint32_t radius;           // distance_radius(max_d2)
    uint8_t* out_pos;          // emitting: 6 bytes per voxel at the scanned offsets; nullptr: counting
    uint8_t* out_mrgb;         // 4 bytes per voxel, or nullptr
    uint8_t* out_d2;           // 2 bytes per voxel, or nullptr
};

// Counting (a.out_pos == nullptr): part[b] = the cells of tile tiles[b] that rule 6 puts into the result.  Emitting: those cells'
// positions, bytes and d2 at part[b] onward in path order, by byte stores: any alignment.
hipError_t launch_distance(const DistanceArgs& a, hipStream_t s);

}  // namespace vxrt
