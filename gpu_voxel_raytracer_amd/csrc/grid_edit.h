// grid_edit.h — what api_grid_edit.hip (host side of vxrt_grid_edit.h) and grid_edit.hip (its kernels) share.  DESIGN.md §13.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "edit.h"
#include "grid.h"
#include "../../include/vxrt_grid_edit.h"

namespace vxrt {

// A grid written into a box of the scene: g is the grid (its box o + [0, n)) with the tiles of the part of the box inside the root
// cube, [clo, chi); for depth < 4 the root cube is the one tile (small = 1), staged from p = -2^depth.
struct GridEdit {
    GridDesc g;
    const SvoRecord* svo;
    const int32_t* leaves;
    uint32_t depth;
    uint32_t mode;        // vxrt_grid_edit_mode
    uint32_t small;
    int32_t clo[3], chi[3];
};

// The two lists of a grid edit, cut into segments on the device and ready for apply_edit_batch: the clears, then the sets.  Every
// device array lives in `buf`.
struct GridEditLists {
    uint64_t set = 0, cleared = 0;
    EditBatch clears, sets;
    ScratchBuffer buf[4];
};

// The diff of the grid against the scene, on `stream` behind what is enqueued there.  `outside`: the sub-boxes of the grid (in grid
// indices: i0, j0, k0, ni, nj, nk) that lie outside the root cube and must hold no occupied cell (SET, REPLACE), up to 6.  Waits
// for the result.  VXRT_E_SCENE: an occupied cell outside the cube, 2^32 sets or clears or more; VXRT_E_DEVICE: an allocation
// failed.  Nothing in the scene changes.
int diff_grid_device(const GridEdit& e, const uint32_t* pal, const uint64_t (*outside)[6], uint32_t n_outside, hipStream_t stream,
                     GridEditLists* out);

}  // namespace vxrt
