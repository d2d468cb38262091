// grid.h — what api_grid.hip (host side of vxrt_grid.h) and grid_build.hip (its kernels) share.  DESIGN.md §12.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_build.h"

namespace vxrt {

// A dense grid of cells in device memory, C order [x][y][z] (z fastest): cell (i, j, k) is the voxel position o + (i, j, k).
// format 1: uint8 palette indices (0 empty); 2: uint32 cells (bit 31 set: the cell is the leaf word; clear: empty).
struct GridDesc {
    const void* cells;
    uint32_t format;
    int32_t o[3];      // origin
    uint32_t n[3];     // dims, each >= 1
    int32_t t0[3];     // the first 16-aligned tile per axis: floor(o / 16)
    uint32_t nt[3];    // tiles per axis
};

// The scene of the grid's occupied cells, exactly as build_svo_device_list builds it from them as a list.  pal: for format 1, 256
// leaf words in device memory (entry 0 = 0).  The grid is read on `stream` behind what is enqueued there; waits for the result.
// VXRT_E_SCENE: 2^32 occupied cells or more, or 2^32 records or more; VXRT_E_DEVICE: an allocation failed.  Nothing is allocated on
// failure.
int build_svo_device_grid(const GridDesc& g, const uint32_t* pal, hipStream_t stream, DeviceTree* out);

// Enqueues on `stream`: cells[(i * n1 + j) * n2 + k] = the leaf word of the voxel at o + (i, j, k), 0 where there is none (outside
// the root cube [-2^depth, 2^depth)^3 included).  n0 * n1 * n2 > 0.
hipError_t launch_grid_export(const SvoRecord* svo, const int32_t* leaves, uint32_t depth, const int32_t o[3], const uint32_t n[3],
                              uint32_t* cells, hipStream_t stream);

}  // namespace vxrt
