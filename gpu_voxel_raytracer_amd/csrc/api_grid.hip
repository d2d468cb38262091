// api_grid.hip — host side of vxrt_grid.h: a dense grid in device memory -> the context's scene (grid_build.hip), installed as
// vxrt_set_voxels_device installs its tree; and a box of the scene -> a dense grid of leaf words.  DESIGN.md §12.
#include "ctx.h"
#include "grid.h"
#include "scene_args.h"
#include "../../include/vxrt_grid.h"

extern "C" {

int vxrt_set_voxel_grid(vxrt_ctx* c, const void* cells, vxrt_grid_format format, const uint32_t dims[3], const int32_t origin[3],
                        const uint8_t (*palette)[4]) try {
    using namespace vxrt;
    if (!valid_ctx(c) || !dims || !origin) { set_error("null argument"); return VXRT_E_INVALID; }
    if (int rc = check_grid_format(format, "vxrt_set_voxel_grid")) return rc;
    if (int rc = check_grid_palette(format, palette, "vxrt_set_voxel_grid")) return rc;
    for (int ax = 0; ax < 3; ax++) {
        if (int64_t(origin[ax]) < -32768 || int64_t(origin[ax]) + int64_t(dims[ax]) > 32768) {
            set_error("vxrt_set_voxel_grid: the grid's box leaves the int16 range");
            return VXRT_E_INVALID;
        }
    }
    size_t bytes = 0;   // < 2^50: the box lies in the int16 range
    if (int rc = check_grid_cells(cells, format, dims, "vxrt_set_voxel_grid", &bytes)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (bytes != 0)
        if (int rc = check_device_array(c, cells, bytes, "vxrt_set_voxel_grid", "cells")) return rc;
    // the old scene may still be read by frames in flight: drain them before it is replaced (this also orders the build behind
    // everything enqueued on the context's stream, vxrt_context_wait_stream's events included)
    if (int rc = sync_all(c)) return rc;
    DeviceTree t;
    if (bytes == 0) {
        if (int rc = build_empty_tree(c->stream, "vxrt_set_voxel_grid", &t)) return rc;
    } else {
        GridDesc g{};
        g.cells = cells;
        g.format = uint32_t(format);
        for (int ax = 0; ax < 3; ax++) {
            g.o[ax] = origin[ax];
            g.n[ax] = dims[ax];
            g.t0[ax] = origin[ax] >> 4;   // floor(origin / 16)
            g.nt[ax] = uint32_t(((origin[ax] + int32_t(dims[ax]) - 1) >> 4) - g.t0[ax] + 1);
        }
        ScratchBuffer pal;
        if (int rc = upload_palette(palette, c->stream, "vxrt_set_voxel_grid", &pal)) return rc;
        if (int rc = build_svo_device_grid(g, pal.as<uint32_t>(), c->stream, &t)) return rc;
    }
    return install_device_tree(c, t, "vxrt_set_voxel_grid");
} VXRT_CATCH

int vxrt_get_voxel_grid(vxrt_ctx* c, const int32_t origin[3], const uint32_t dims[3], uint32_t* cells) try {
    using namespace vxrt;
    if (!valid_ctx(c) || !origin || !dims) { set_error("null argument"); return VXRT_E_INVALID; }
    unsigned __int128 bytes = 4;
    for (int ax = 0; ax < 3; ax++) bytes *= dims[ax];
    if (bytes >> 64) { set_error("vxrt_get_voxel_grid: a box of 2^64 bytes or more"); return VXRT_E_INVALID; }
    if (bytes == 0) return VXRT_OK;
    if (!cells) { set_error("vxrt_get_voxel_grid: null cells"); return VXRT_E_INVALID; }
    if (int rc = require_scene(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_device_array(c, cells, size_t(bytes), "vxrt_get_voxel_grid", "cells")) return rc;
    HIP_TRY(launch_grid_export(c->d_svo, c->d_leaves, c->depth, origin, dims, cells, c->stream));
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
