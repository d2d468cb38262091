// api_components.hip — host side of vxrt_components.h: the connected components of a voxel list in device memory, and the voxels of
// the loaded scene that hang on nothing inside an anchor box.  The sort and the scans are the list builder's (device_build.h), the
// scene's list is vxrt_get_voxels_device's (api_extract.hip), everything between is components.hip.  Nothing but counts crosses to
// the host: the unique voxels, the components, and for the scene call the scene's and the detached voxels.  DESIGN.md §20.
#include <string>

#include "components.h"
#include "ctx.h"
#include "device_build.h"
#include "scene_args.h"
#include "../../include/vxrt_components.h"
#include "../../include/vxrt_device_edit.h"

namespace vxrt {

// About 40 bytes per entry, all of it allocated before the first launch.
int alloc_labelling(size_t n, const char* who, Labelling* l) {
    if (int rc = alloc_list_scratch(n, true, who, &l->ls)) return rc;
    for (ScratchBuffer* b : {&l->uhead, &l->parent, &l->comp, &l->acc})
        if (int rc = alloc_scratch(b, n * sizeof(uint32_t), who, "the union-find")) return rc;
    return alloc_scratch(&l->part, (size_t(comp_blocks(n)) + 1) * sizeof(uint64_t), who, "the scan partials");
}

// pos[0 .. n), 0 < n < 2^32, read on s -> *l.  axes: 1, 2 or 3.  Waits for the two counts.
int label_list(const int16_t* pos, uint32_t n, uint32_t axes, const CompBox& box, hipStream_t s, Labelling* l) {
    uint64_t* kp[2] = {l->ls.keys[0].as<uint64_t>(), l->ls.keys[1].as<uint64_t>()};
    uint32_t* vp[2] = {l->ls.vals[0].as<uint32_t>(), l->ls.vals[1].as<uint32_t>()};
    uint64_t* part = l->part.as<uint64_t>();
    HIP_TRY(components_keys(pos, n, kp[0], vp[0], s));
    int cur = 0;
    HIP_TRY(radix_sort_pairs(kp, vp, n, kCompKeyBits, l->ls.hist.as<uint32_t>(), l->ls.totals.as<uint32_t>(), s, &cur));
    // the sort's other buffers are free from here on: they take the unique keys and the entries' ranks
    uint64_t* ukeys = kp[cur ^ 1];
    uint32_t* rank = vp[cur ^ 1];
    HIP_TRY(components_heads_count(kp[cur], n, part, s));
    HIP_TRY(launch_exclusive_scan(part, comp_blocks(n), s));
    uint64_t m = 0;
    HIP_TRY(hipMemcpyAsync(&m, part + comp_blocks(n), sizeof m, hipMemcpyDeviceToHost, s));
    HIP_TRY(components_heads_write(kp[cur], vp[cur], n, part, ukeys, l->uhead.as<uint32_t>(), rank, l->parent.as<uint32_t>(), l->acc.as<uint32_t>(), s));
    HIP_TRY(hipStreamSynchronize(s));      // m; the partials are rewritten below
    const uint32_t mm = uint32_t(m);       // 0 < m <= n
    HIP_TRY(components_union(ukeys, mm, axes, l->parent.as<uint32_t>(), s));
    HIP_TRY(components_flatten(ukeys, l->uhead.as<uint32_t>(), l->parent.as<uint32_t>(), mm, box, l->comp.as<uint32_t>(), l->acc.as<uint32_t>(), part, s));
    HIP_TRY(launch_exclusive_scan(part, comp_blocks(mm), s));
    HIP_TRY(hipMemcpyAsync(&l->components, part + comp_blocks(mm), sizeof l->components, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    l->ukeys = ukeys;
    l->sorted = vp[cur];
    l->rank = rank;
    l->unique = mm;
    return VXRT_OK;
}

// 6, 18, 26 -> the axes on which two neighbours may differ; anything else -> 0
uint32_t axes_of(uint32_t connectivity) { return connectivity == 6u ? 1u : connectivity == 18u ? 2u : connectivity == 26u ? 3u : 0u; }

}  // namespace vxrt

extern "C" {

int vxrt_label_components_device(vxrt_ctx* c, const int16_t (*pos)[3], size_t n, uint32_t connectivity, uint32_t* label,
                                 size_t* n_components) try {
    using namespace vxrt;
    const char* who = "vxrt_label_components_device";
    if (!valid_ctx(c) || !n_components) { set_error("null argument"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error(std::string(who) + ": 2^32 voxels or more"); return VXRT_E_INVALID; }
    const uint32_t axes = axes_of(connectivity);
    if (axes == 0u) { set_error(std::string(who) + ": connectivity " + std::to_string(connectivity) + " (6, 18 or 26)"); return VXRT_E_INVALID; }
    if (n == 0) { *n_components = 0; return VXRT_OK; }
    if (!pos) { set_error(std::string(who) + ": null voxel positions"); return VXRT_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(label) & 3u) != 0u) { set_error(std::string(who) + ": label must be 4-byte aligned"); return VXRT_E_INVALID; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_device_array(c, pos, n * 3 * sizeof(int16_t), who, "pos")) return rc;
    if (label)
        if (int rc = check_device_array(c, label, n * sizeof(uint32_t), who, "label")) return rc;

    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    Labelling l;
    if (int rc = alloc_labelling(n, who, &l)) return rc;
    CompBox box{};
    if (int rc = label_list(reinterpret_cast<const int16_t*>(pos), uint32_t(n), axes, box, s, &l)) return rc;
    if (label) {
        HIP_TRY(components_scatter(l.sorted, l.rank, uint32_t(n), l.comp.as<uint32_t>(), l.acc.as<uint32_t>(), 0u, label, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    *n_components = size_t(l.components);
    return VXRT_OK;
} VXRT_CATCH

int vxrt_detached_voxels_device(vxrt_ctx* c, const int32_t anchor_min[3], const int32_t anchor_max[3], uint32_t connectivity,
                                int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap, size_t* n) try {
    using namespace vxrt;
    const char* who = "vxrt_detached_voxels_device";
    if (!valid_ctx(c) || !n) { set_error("null argument"); return VXRT_E_INVALID; }
    if (!anchor_min || !anchor_max) { set_error(std::string(who) + ": null anchor box"); return VXRT_E_INVALID; }
    const uint32_t axes = axes_of(connectivity);
    if (axes == 0u) { set_error(std::string(who) + ": connectivity " + std::to_string(connectivity) + " (6, 18 or 26)"); return VXRT_E_INVALID; }
    if ((pos == nullptr) != (mrgb == nullptr)) { set_error("pos and mrgb: both or neither"); return VXRT_E_INVALID; }
    if (int rc = require_scene(c)) return rc;
    const bool count_only = pos == nullptr;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (!count_only && cap != 0) {
        if (int rc = check_device_array(c, pos, cap * 3 * sizeof(int16_t), who, "pos")) return rc;
        if (int rc = check_device_array(c, mrgb, cap * 4, who, "mrgb")) return rc;
    }

    // the scene's list, in path order, into scratch: counted, then decoded
    size_t total = 0;
    if (int rc = vxrt_get_voxels_device(c, nullptr, nullptr, nullptr, nullptr, 0, &total)) return rc;
    if (total == 0) { *n = 0; return VXRT_OK; }
    const uint32_t nn = uint32_t(total);   // a scene holds fewer than 2^32 leaf words
    ScratchBuffer spos, smrgb, flag;
    Labelling l;
    if (int rc = alloc_scratch(&spos, total * 3 * sizeof(int16_t), who, "the scene's positions")) return rc;
    if (int rc = alloc_scratch(&smrgb, total * 4, who, "the scene's mrgb words")) return rc;
    if (int rc = alloc_scratch(&flag, total * sizeof(uint32_t), who, "the flags")) return rc;
    if (int rc = alloc_labelling(total, who, &l)) return rc;
    size_t got = 0;
    if (int rc = vxrt_get_voxels_device(c, nullptr, nullptr, reinterpret_cast<int16_t(*)[3]>(spos.p), reinterpret_cast<uint8_t(*)[4]>(smrgb.p), total, &got))
        return rc;

    hipStream_t s = c->stream;
    CompBox box{};
    for (int ax = 0; ax < 3; ax++) { box.lo[ax] = anchor_min[ax]; box.hi[ax] = anchor_max[ax]; }
    box.on = 1u;
    if (int rc = label_list(spos.as<int16_t>(), nn, axes, box, s, &l)) return rc;
    uint64_t* part = l.part.as<uint64_t>();
    HIP_TRY(components_scatter(l.sorted, l.rank, nn, l.comp.as<uint32_t>(), l.acc.as<uint32_t>(), 1u, flag.as<uint32_t>(), s));
    HIP_TRY(components_select_count(flag.as<uint32_t>(), nn, part, s));
    HIP_TRY(launch_exclusive_scan(part, comp_blocks(nn), s));
    uint64_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, part + comp_blocks(nn), sizeof count, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (count_only || count == 0) { *n = size_t(count); return VXRT_OK; }
    if (cap < count) {
        *n = size_t(count);
        set_error(std::string(who) + ": " + std::to_string(count) + " voxels, room for " + std::to_string(cap));
        return VXRT_E_INVALID;
    }
    // written in place where the kernel's stores fit the arrays' alignment (2 bytes per coordinate, 4 per mrgb word); otherwise
    // staged and copied
    const bool direct = (reinterpret_cast<uintptr_t>(pos) & 1u) == 0u && (reinterpret_cast<uintptr_t>(mrgb) & 3u) == 0u;
    ScratchBuffer dpos, dmrgb;
    if (!direct) {
        if (int rc = alloc_scratch(&dpos, size_t(count) * 3 * sizeof(int16_t), who, "the positions")) return rc;
        if (int rc = alloc_scratch(&dmrgb, size_t(count) * 4, who, "the mrgb words")) return rc;
    }
    HIP_TRY(components_select_write(flag.as<uint32_t>(), nn, part, spos.as<int16_t>(), smrgb.as<uint32_t>(),
                                    direct ? reinterpret_cast<int16_t*>(pos) : dpos.as<int16_t>(),
                                    direct ? reinterpret_cast<uint32_t*>(mrgb) : dmrgb.as<uint32_t>(), s));
    if (!direct) {
        HIP_TRY(hipMemcpyAsync(pos, dpos.p, size_t(count) * 3 * sizeof(int16_t), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(mrgb, dmrgb.p, size_t(count) * 4, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    *n = size_t(count);
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
