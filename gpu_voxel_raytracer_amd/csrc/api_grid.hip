// api_grid.hip — host side of vxrt_grid.h: a dense grid in device memory -> the context's scene (grid_build.hip), installed as
// vxrt_set_voxels_device installs its tree; and a box of the scene -> a dense grid of leaf words.  DESIGN.md §12.
#include "ctx.h"
#include "grid.h"
#include "../../include/vxrt_grid.h"

extern "C" {

int vxrt_set_voxel_grid(vxrt_ctx* c, const void* cells, vxrt_grid_format format, const uint32_t dims[3], const int32_t origin[3],
                        const uint8_t (*palette)[4]) try {
    using namespace vxrt;
    if (!valid_ctx(c) || !dims || !origin) { set_error("null argument"); return VXRT_E_INVALID; }
    if (format != VXRT_GRID_PALETTE8 && format != VXRT_GRID_WORD32) { set_error("vxrt_set_voxel_grid: bad format"); return VXRT_E_INVALID; }
    if ((format == VXRT_GRID_PALETTE8) != (palette != nullptr)) {
        set_error("vxrt_set_voxel_grid: a palette is required for PALETTE8 cells and refused for WORD32 cells");
        return VXRT_E_INVALID;
    }
    uint64_t count = 1;
    for (int ax = 0; ax < 3; ax++) {
        if (int64_t(origin[ax]) < -32768 || int64_t(origin[ax]) + int64_t(dims[ax]) > 32768) {
            set_error("vxrt_set_voxel_grid: the grid's box leaves the int16 range");
            return VXRT_E_INVALID;
        }
        count *= dims[ax];   // <= 2^48
    }
    if (count != 0 && !cells) { set_error("vxrt_set_voxel_grid: null cells"); return VXRT_E_INVALID; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    const size_t cell_bytes = format == VXRT_GRID_PALETTE8 ? 1 : 4;
    if (count != 0)
        if (int rc = check_device_array(c, cells, size_t(count) * cell_bytes, "vxrt_set_voxel_grid", "cells")) return rc;
    // the old scene may still be read by frames in flight: drain them before it is replaced (this also orders the build behind
    // everything enqueued on the context's stream, vxrt_context_wait_stream's events included)
    if (int rc = sync_all(c)) return rc;
    DeviceTree t;
    if (count == 0) {
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
        if (format == VXRT_GRID_PALETTE8) {   // the palette as leaf words (scene_host.cpp: build_octree's rule); index 0 is empty
            uint32_t words[256];
            words[0] = 0u;
            for (int i = 1; i < 256; i++)
                words[i] = 0x80000000u | (uint32_t(palette[i][0]) & 0x7fu) << 24 | uint32_t(palette[i][1]) << 16 |
                           uint32_t(palette[i][2]) << 8 | uint32_t(palette[i][3]);
            if (hipError_t e = pal.alloc(sizeof words); e != hipSuccess) {
                (void)hipGetLastError();
                pal.p = nullptr;
                return hip_fail(e, "vxrt_set_voxel_grid: allocating the palette");
            }
            HIP_TRY(hipMemcpyAsync(pal.p, words, sizeof words, hipMemcpyHostToDevice, c->stream));
        }
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
    if (!c->has_scene || c->d_svo == nullptr || c->d_leaves == nullptr) { set_error("no scene set"); return VXRT_E_NOSCENE; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_device_array(c, cells, size_t(bytes), "vxrt_get_voxel_grid", "cells")) return rc;
    HIP_TRY(launch_grid_export(c->d_svo, c->d_leaves, c->depth, origin, dims, cells, c->stream));
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
