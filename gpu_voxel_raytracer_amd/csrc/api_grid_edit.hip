// api_grid_edit.hip — host side of vxrt_grid_edit.h: a dense grid in device memory written into a box of the scene.  The diff, the
// two lists and their segments are made on the device (grid_edit.hip); the lists are applied by the tail vxrt_edit_voxels uses
// (api_edit.hip: apply_edit_batch), clears first.  DESIGN.md §13.
#include <algorithm>

#include "ctx.h"
#include "grid_edit.h"
#include "scene_args.h"
#include "../../include/vxrt_grid_edit.h"

namespace vxrt {
namespace {

// the sub-boxes of the box o + [0, n) outside the cube [-h, h)^3, in grid indices {i0, j0, k0, ni, nj, nk}: the slabs below and
// above the cube along x, then along y within the cube's x range, then along z within both
uint32_t outside_slabs(const int32_t o[3], const uint32_t n[3], int64_t h, uint64_t slabs[6][6]) {
    uint32_t count = 0;
    uint64_t lo[3] = {0, 0, 0}, cnt[3] = {n[0], n[1], n[2]};   // the part of the box inside the cube on the axes done so far
    for (int ax = 0; ax < 3; ax++) {
        const int64_t a = std::max<int64_t>(o[ax], -h) - o[ax], b = std::min<int64_t>(int64_t(o[ax]) + n[ax], h) - o[ax];
        auto add = [&](uint64_t from, uint64_t len) {
            if (len == 0) return;
            uint64_t* s = slabs[count++];
            for (int k = 0; k < 3; k++) { s[k] = lo[k]; s[3 + k] = cnt[k]; }
            s[ax] = from;
            s[3 + ax] = len;
        };
        if (a >= b) {   // nothing of the box is inside the cube along this axis
            add(0, n[ax]);
            return count;
        }
        add(0, uint64_t(a));
        add(uint64_t(b), n[ax] - uint64_t(b));
        lo[ax] = uint64_t(a);
        cnt[ax] = uint64_t(b - a);
    }
    return count;
}

}  // namespace
}  // namespace vxrt

extern "C" {

int vxrt_edit_voxel_grid(vxrt_ctx* c, const void* cells, vxrt_grid_format format, const uint32_t dims[3], const int32_t origin[3],
                         const uint8_t (*palette)[4], vxrt_grid_edit_mode mode, vxrt_grid_edit_counts* counts) try {
    using namespace vxrt;
    if (counts) *counts = vxrt_grid_edit_counts{0, 0};
    if (!valid_ctx(c) || !dims || !origin) { set_error("null argument"); return VXRT_E_INVALID; }
    if (int rc = check_grid_format(format, "vxrt_edit_voxel_grid")) return rc;
    if (mode != VXRT_GRID_EDIT_REPLACE && mode != VXRT_GRID_EDIT_SET && mode != VXRT_GRID_EDIT_CLEAR) {
        set_error("vxrt_edit_voxel_grid: bad mode");
        return VXRT_E_INVALID;
    }
    if (int rc = check_grid_palette(format, palette, "vxrt_edit_voxel_grid")) return rc;
    size_t bytes = 0;
    if (int rc = check_grid_cells(cells, format, dims, "vxrt_edit_voxel_grid", &bytes)) return rc;
    if (int rc = require_scene(c)) return rc;
    if (int rc = require_editable_scene(c)) return rc;
    if (bytes == 0) return VXRT_OK;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_device_array(c, cells, bytes, "vxrt_edit_voxel_grid", "cells")) return rc;
    // frames in flight read the scene: drain them first (this also orders the reads behind everything enqueued on the context's
    // stream, vxrt_context_wait_stream's events included)
    if (int rc = sync_all(c)) return rc;

    const uint32_t L = c->depth;
    const int64_t h = int64_t(1) << L;
    GridEdit e{};
    e.g.cells = cells;
    e.g.format = uint32_t(format);
    e.svo = c->d_svo;
    e.leaves = c->d_leaves;
    e.depth = L;
    e.mode = uint32_t(mode);
    e.small = L < 4u ? 1u : 0u;
    bool inside = true, meets = true;   // the box lies inside the root cube / meets it
    for (int ax = 0; ax < 3; ax++) {
        e.g.o[ax] = origin[ax];
        e.g.n[ax] = dims[ax];
        const int64_t lo = std::max<int64_t>(origin[ax], -h), hi = std::min<int64_t>(int64_t(origin[ax]) + dims[ax], h);
        inside = inside && lo == origin[ax] && hi == int64_t(origin[ax]) + dims[ax];
        meets = meets && lo < hi;
        e.clo[ax] = int32_t(lo);
        e.chi[ax] = int32_t(std::max(lo, hi));
        // the 16-aligned tiles of box ∩ cube (d >= 4); for d < 4 the root cube is the one tile
        e.g.t0[ax] = int32_t(lo) >> 4;
        e.g.nt[ax] = lo < hi ? uint32_t(((int32_t(hi) - 1) >> 4) - e.g.t0[ax] + 1) : 0u;
        if (e.small) e.g.nt[ax] = lo < hi ? 1u : 0u;
    }
    if (!meets)
        for (int ax = 0; ax < 3; ax++) e.g.nt[ax] = 0;
    uint64_t slabs[6][6];
    const uint32_t n_slabs = mode != VXRT_GRID_EDIT_CLEAR && !inside ? outside_slabs(origin, dims, h, slabs) : 0u;

    ScratchBuffer pal;
    if (int rc = upload_palette(palette, c->stream, "vxrt_edit_voxel_grid", &pal)) return rc;
    GridEditLists lists;
    if (int rc = diff_grid_device(e, pal.as<uint32_t>(), slabs, n_slabs, c->stream, &lists)) return rc;
    if (lists.set == 0 && lists.cleared == 0) return VXRT_OK;
    // all or nothing: the sets' storage is reserved before the clears change the scene (a clear never grows it)
    if (lists.set) {
        const EditBatch& s = lists.sets;
        if (int rc = reserve_edit_storage(c, s.seg_off[L], s.seg_off[L + 1] - s.seg_off[L])) return rc;
    }
    if (lists.cleared)
        if (int rc = apply_edit_batch(c, lists.clears)) return rc;
    if (lists.set)
        if (int rc = apply_edit_batch(c, lists.sets)) return rc;
    if (counts) *counts = vxrt_grid_edit_counts{lists.set, lists.cleared};
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
