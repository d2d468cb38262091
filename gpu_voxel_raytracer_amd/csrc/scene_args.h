// scene_args.h — the host-side argument checks of the scene extensions (vxrt_device_scene.h, vxrt_extract.h, vxrt_edit.h,
// vxrt_grid.h, vxrt_grid_edit.h) and the palette upload of the two grid calls.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "ctx.h"
#include "../../include/vxrt_grid.h"

namespace vxrt {

// `bytes` at p must be device memory of the context's device, inside one allocation.  who: the API call.
inline int check_device_array(const vxrt_ctx* c, const void* p, size_t bytes, const char* who, const char* what) {
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        set_error(std::string(who) + ": " + what + " is not device memory");
        return VXRT_E_INVALID;
    }
    if (a.type != hipMemoryTypeDevice || a.device != c->cfg.device) {
        set_error(std::string(who) + ": " + what + " is not device memory of the context's device");
        return VXRT_E_INVALID;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) == hipSuccess) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(base), at = reinterpret_cast<uintptr_t>(p);
        if (at - lo > size || bytes > size - (at - lo)) {
            set_error(std::string(who) + ": " + what + " ends past its allocation");
            return VXRT_E_INVALID;
        }
    } else {
        (void)hipGetLastError();
    }
    return VXRT_OK;
}

// A scene is loaded and its 8-byte records and leaf words are on the device.
inline int require_scene(const vxrt_ctx* c) {
    if (!c->has_scene || c->d_svo == nullptr || c->d_leaves == nullptr) { set_error("no scene set"); return VXRT_E_NOSCENE; }
    return VXRT_OK;
}

// The scene can be edited in place: 8-byte records only, in breadth-first order.
inline int require_editable_scene(const vxrt_ctx* c) {
    if (c->d_wide != nullptr || c->scene_format == 1) { set_error("scene edits need the 8-byte records only (VXRT_OPT_SCENE_FORMAT 0)"); return VXRT_E_INVALID; }
    if (c->node_order_applied != 0) { set_error("scene edits need the breadth-first records (VXRT_OPT_NODE_ORDER 0)"); return VXRT_E_INVALID; }
    return VXRT_OK;
}

// The argument checks vxrt_set_voxel_grid and vxrt_edit_voxel_grid share, in the order each call runs them between its own: the
// format; the palette (present exactly for PALETTE8 cells); the box's byte count (< 2^64, -> *bytes) and the cells (non-null unless
// the box is empty).  who: the API call.
inline int check_grid_format(vxrt_grid_format format, const char* who) {
    if (format != VXRT_GRID_PALETTE8 && format != VXRT_GRID_WORD32) { set_error(std::string(who) + ": bad format"); return VXRT_E_INVALID; }
    return VXRT_OK;
}

inline int check_grid_palette(vxrt_grid_format format, const uint8_t (*palette)[4], const char* who) {
    if ((format == VXRT_GRID_PALETTE8) != (palette != nullptr)) {
        set_error(std::string(who) + ": a palette is required for PALETTE8 cells and refused for WORD32 cells");
        return VXRT_E_INVALID;
    }
    return VXRT_OK;
}

inline int check_grid_cells(const void* cells, vxrt_grid_format format, const uint32_t dims[3], const char* who, size_t* bytes) {
    unsigned __int128 n = format == VXRT_GRID_PALETTE8 ? 1 : 4;
    for (int ax = 0; ax < 3; ax++) n *= dims[ax];
    if (n >> 64) { set_error(std::string(who) + ": a box of 2^64 bytes or more"); return VXRT_E_INVALID; }
    if (n != 0 && !cells) { set_error(std::string(who) + ": null cells"); return VXRT_E_INVALID; }
    *bytes = size_t(n);
    return VXRT_OK;
}

// The palette as 256 leaf words in device memory (scene_host.cpp: build_octree's rule; index 0 is empty), copied on `stream`; none
// for a null palette.  who: the API call.
inline int upload_palette(const uint8_t (*palette)[4], hipStream_t stream, const char* who, ScratchBuffer* out) {
    if (!palette) return VXRT_OK;
    uint32_t words[256];
    words[0] = 0u;
    for (int i = 1; i < 256; i++)
        words[i] = 0x80000000u | (uint32_t(palette[i][0]) & 0x7fu) << 24 | uint32_t(palette[i][1]) << 16 | uint32_t(palette[i][2]) << 8 |
                   uint32_t(palette[i][3]);
    if (int rc = alloc_scratch(out, sizeof words, who, "the palette")) return rc;
    HIP_TRY(hipMemcpyAsync(out->get(), words, sizeof words, hipMemcpyHostToDevice, stream));
    return VXRT_OK;
}

}  // namespace vxrt
