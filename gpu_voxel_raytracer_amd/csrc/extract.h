// extract.h — what api_extract.hip (host side of vxrt_extract.h) and extract.hip (its kernels) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace vxrt {

// The decode is level-synchronous: the frontier of node level l holds, in octree path order, one entry per node of that level whose
// cube meets the box — {record index, u.x, u.y, u.z} with u the node's integer cell (l bits per axis; the root is {0, 0, 0, 0}).
// Each level is three launches over the frontier, in blocks of kExtractSpan entries:
//   extract_count  per block: the number of kept children (or voxels, at the leaf parents' level) -> part[block]
//   exclusive_scan one workgroup: part[] -> its exclusive prefix sum in place, the total -> part[blocks] (device_build.h)
//   extract_expand the kept children, written at their exclusive-prefix offsets (the next frontier), or at the leaf parents'
//                  level the voxels (positions and mrgb)
// Every offset is a prefix sum in frontier order; nothing is decided by an atomic, so two calls write the same bytes.
constexpr uint32_t kExtractThreads = 256;
constexpr uint32_t kExtractItems = 8;                                   // entries per thread
constexpr uint32_t kExtractSpan = kExtractThreads * kExtractItems;      // entries per block

struct ExtractLevel {
    const SvoRecord* svo;
    const int32_t* leaves;
    const uint4* front;       // this level's frontier: n entries
    uint32_t n;
    uint32_t leaf;            // 1: this is the level of the leaf parents (the tree's depth): the leaf mask gives the voxels
    uint32_t shift;           // a child's cube spans 2^shift cells of the voxel grid per axis (depth - level)
    uint32_t half;            // 2^depth: voxel position = u - half
    uint32_t lo[3], hi[3];    // the box on the voxel grid u = p + half, clamped to [0, 2^(depth+1)), lo < hi
    uint64_t* part;           // per block of the frontier, then the total
    uint4* next;              // node levels: the next frontier
    int16_t* pos;             // leaf parents' level: the voxels' positions (3 per voxel) ...
    uint32_t* mrgb;           // ... and (material, r, g, b) bytes
};

hipError_t launch_extract_count(const ExtractLevel& a, hipStream_t s);
hipError_t launch_extract_expand(const ExtractLevel& a, hipStream_t s);

inline uint32_t extract_blocks(uint32_t n) { return (n + kExtractSpan - 1) / kExtractSpan; }

}  // namespace vxrt
