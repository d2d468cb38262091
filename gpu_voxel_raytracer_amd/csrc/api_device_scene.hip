// api_device_scene.hip — host side of vxrt_device_scene.h: a voxel list in device memory -> the context's scene, built on the device
// (device_build.hip) and installed like the procedural scene (api_scene.hip: install_scene).  DESIGN.md §11.
#include "ctx.h"
#include "device_build.h"
#include "scene_args.h"
#include "../../include/vxrt_device_scene.h"

namespace vxrt {

int install_device_tree(vxrt_ctx* c, const DeviceTree& t, const char* who) {
    DeviceBuf<SvoRecord> svo;   // owned here until installed
    DeviceBuf<int32_t> leaves;
    DeviceBuf<WideRec> wide;
    svo.adopt(t.svo);
    leaves.adopt(t.leaves);
    size_t nwide = 0;
    WideRec wide_root{0, 0, 0, 0};
    if (c->scene_format == 1) {   // the wide records (variants only): from the built records on the host, as upload_svo makes them
        std::vector<SvoRecord> recs(t.svo_count);
        HIP_TRY(hipMemcpy(recs.data(), t.svo, t.svo_count * sizeof(SvoRecord), hipMemcpyDeviceToHost));
        std::vector<WideRec> w;
        if (int rc = widen_svo(recs, t.depth, &w)) return rc;
        if (hipError_t e = wide.alloc(w.size()); e != hipSuccess) return alloc_failed(e, who, "the wide records");
        HIP_TRY(hipMemcpy(wide, w.data(), w.size() * sizeof(WideRec), hipMemcpyHostToDevice));
        nwide = w.size();
        wide_root = w[0];
    }
    return install_scene(c, std::move(svo), t.svo_count, std::move(leaves), t.leaf_count, t.depth, t.root, std::move(wide), nwide, wide_root);
}

}  // namespace vxrt

extern "C" {

int vxrt_set_voxels_device(vxrt_ctx* c, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n) try {
    if (!valid_ctx(c)) return VXRT_E_INVALID;
    if (n != 0 && (!pos || !mrgb)) { set_error("null voxel arrays"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error("vxrt_set_voxels_device: 2^32 voxels or more"); return VXRT_E_INVALID; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (n != 0) {
        if (int rc = check_device_array(c, pos, n * 3 * sizeof(int16_t), "vxrt_set_voxels_device", "pos")) return rc;
        if (int rc = check_device_array(c, mrgb, n * 4, "vxrt_set_voxels_device", "mrgb")) return rc;
    }
    // the old scene may still be read by frames in flight: drain them before it is replaced (this also orders the build behind
    // everything enqueued on the context's stream, vxrt_context_wait_stream's events included)
    if (int rc = sync_all(c)) return rc;
    DeviceTree t;
    if (int rc = build_svo_device_list(reinterpret_cast<const int16_t*>(pos), reinterpret_cast<const uint8_t*>(mrgb), n, c->stream, &t)) return rc;
    return install_device_tree(c, t, "vxrt_set_voxels_device");
} VXRT_CATCH

}  // extern "C"
