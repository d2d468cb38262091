// api_device_edit.hip — host side of vxrt_device_edit.h: vxrt_edit_voxels with the list in device memory.  One pass keys the list at
// the scene's depth (device_edit.hip), the list builder's front sorts and dedupes it (device_build.hip: sort_unique_list), the grid
// editor's cut makes edit_kernel's segments (grid_edit.hip: cut_edit_lists), and the tail is vxrt_edit_voxels' own (api_edit.hip:
// apply_edit_batch).  vxrt_get_voxels_device is in api_extract.hip, beside the host call it shares everything with.  DESIGN.md §15.
#include <string>

#include "ctx.h"
#include "device_build.h"
#include "edit.h"
#include "scene_args.h"
#include "../../include/vxrt_device_edit.h"

extern "C" {

int vxrt_edit_voxels_device(vxrt_ctx* c, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n) try {
    using namespace vxrt;
    const char* who = "vxrt_edit_voxels_device";
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (n != 0 && !pos) { set_error("null voxel positions"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error(std::string(who) + ": 2^32 voxels or more"); return VXRT_E_INVALID; }
    if (int rc = require_scene(c)) return rc;
    if (n == 0) return VXRT_OK;
    if (int rc = require_editable_scene(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_device_array(c, pos, n * 3 * sizeof(int16_t), who, "pos")) return rc;
    if (mrgb)
        if (int rc = check_device_array(c, mrgb, n * 4, who, "mrgb")) return rc;
    // frames in flight read the scene: drain them first (this also orders the reads behind everything enqueued on the context's
    // stream, vxrt_context_wait_stream's events included)
    if (int rc = sync_all(c)) return rc;

    const bool clear = mrgb == nullptr;
    const uint32_t L = c->depth, nn = uint32_t(n);
    hipStream_t s = c->stream;
    ListScratch ls;
    if (int rc = alloc_list_scratch(n, !clear, who, &ls)) return rc;
    ListBounds lb;
    if (int rc = edit_keys_device(reinterpret_cast<const int16_t*>(pos), reinterpret_cast<const uint8_t*>(mrgb), n, L,
                                  ls.keys(), ls.vals(), s, who, &lb))
        return rc;
    if (lb.outside) {
        const std::string half = std::to_string(int32_t(1) << L);
        set_error(std::string(who) + ": the positions span [" + std::to_string(lb.lo[0]) + ", " + std::to_string(lb.hi[0]) + "] x [" +
                  std::to_string(lb.lo[1]) + ", " + std::to_string(lb.hi[1]) + "] x [" + std::to_string(lb.lo[2]) + ", " +
                  std::to_string(lb.hi[2]) + "]: outside the scene's root cube [-" + half + ", " + half + ")^3");
        return VXRT_E_SCENE;
    }
    ScratchBuffer words, segments;
    size_t m = 0;
    if (int rc = sort_unique_list(&ls, nn, L, &words, s, who, &m)) return rc;

    EditBatch b;
    const uint64_t* keys[1] = {ls.keys()};
    const uint32_t count[1] = {uint32_t(m)};
    EditBatch* out[1] = {&b};
    if (int rc = cut_edit_lists(keys, count, 1, L, s, who, &segments, out)) return rc;
    b.clear = clear;
    b.words = clear ? nullptr : words.as<int32_t>();
    for (int ax = 0; ax < 3; ax++) { b.lo[ax] = lb.lo[ax]; b.hi[ax] = lb.hi[ax]; }
    return apply_edit_batch(c, b);
} VXRT_CATCH

}  // extern "C"
