// api_extract.hip — host side of vxrt_extract.h: the scene's voxels, whole or by box, decoded on the device (extract.hip).
// The host runs the levels (extract.h) and reads back one number per level, the size of the next frontier, so that the scratch can
// grow to it; the output goes to device buffers and comes back in one copy per array (vxrt_get_voxels), or straight into the caller's
// device arrays (vxrt_get_voxels_device).  DESIGN.md "Reading the scene back", §15.
#include <algorithm>
#include <string>

#include "ctx.h"
#include "device_build.h"
#include "extract.h"
#include "list_ops.h"
#include "scene_args.h"
#include "../../include/vxrt_device_edit.h"
#include "../../include/vxrt_extract.h"

namespace vxrt {
namespace {

// `g` holds at least `need` bytes afterwards; growth is geometric (x 1.5).  A failed allocation leaves the old buffer in place.
// The contents are not kept (every buffer here is written before it is read, within one call).
hipError_t ensure(vxrt_ctx::GrowBuf& g, size_t need) {
    if (need <= g.cap && g.buf) return hipSuccess;
    size_t want = std::max(need, g.cap + g.cap / 2);
    DeviceBuf<void> fresh;
    hipError_t e = fresh.alloc(want);
    if (e != hipSuccess && want != need) {
        (void)hipGetLastError();
        want = need;
        e = fresh.alloc(want);   // the geometric step did not fit: exactly what is needed
    }
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    g.buf.swap(fresh);
    g.cap = want;
    return hipSuccess;
}

}  // namespace

// vxrt_get_voxels (device = false: pos / mrgb are host arrays) and vxrt_get_voxels_device (device memory of the context's device)
static int get_voxels(vxrt_ctx* c, const int32_t box_min[3], const int32_t box_max[3], int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap, size_t* n,
                      bool device, const char* who) {
    if (!valid_ctx(c) || !n) { set_error("null argument"); return VXRT_E_INVALID; }
    if ((box_min == nullptr) != (box_max == nullptr)) { set_error("box_min and box_max: both or neither"); return VXRT_E_INVALID; }
    if ((pos == nullptr) != (mrgb == nullptr)) { set_error("pos and mrgb: both or neither"); return VXRT_E_INVALID; }
    if (int rc = require_scene(c)) return rc;
    const bool count_only = pos == nullptr;
    const uint32_t L = c->depth;
    const int64_t half = int64_t(1) << L;
    // the box on the voxel grid u = p + 2^depth, clamped to the root cube [0, 2^(depth+1))^3
    ExtractLevel a{};
    bool empty = c->svo_count == 0;
    for (int ax = 0; ax < 3; ax++) {
        const int64_t lo = box_min ? std::clamp(int64_t(box_min[ax]) + half, int64_t(0), 2 * half) : 0;
        const int64_t hi = box_max ? std::clamp(int64_t(box_max[ax]) + half, int64_t(0), 2 * half) : 2 * half;
        if (lo >= hi) empty = true;
        a.lo[ax] = uint32_t(lo);
        a.hi[ax] = uint32_t(hi);
    }
    if (empty) { *n = 0; return VXRT_OK; }
    a.svo = c->d_svo;
    a.leaves = c->d_leaves;
    a.half = uint32_t(half);

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (device && !count_only && cap != 0) {
        if (int rc = check_device_array(c, pos, cap * 3 * sizeof(int16_t), who, "pos")) return rc;
        if (int rc = check_device_array(c, mrgb, cap * 4, who, "mrgb")) return rc;
    }
    vxrt_ctx::ExtractScratch& x = c->extract;
    // the root: record 0 at cell 0 (the decode runs on the context's stream, behind everything enqueued on it)
    if (hipError_t e = ensure(x.front[0], sizeof(uint4)); e != hipSuccess) return alloc_failed(e, who, "the frontier");
    HIP_TRY(hipMemsetAsync(x.front[0].buf, 0, sizeof(uint4), c->stream));
    int cur = 0;
    uint64_t count = 0;
    uint32_t frontier = 1;
    for (uint32_t l = 0; l <= L; l++) {
        a.leaf = l == L ? 1u : 0u;
        a.shift = L - l;
        a.front = x.front[cur].buf.as<const uint4>();
        a.n = frontier;
        const uint32_t blocks = extract_blocks(frontier);
        if (hipError_t e = ensure(x.part, (size_t(blocks) + 1) * sizeof(uint64_t)); e != hipSuccess)
            return alloc_failed(e, who, "the scan partials");
        a.part = x.part.buf.as<uint64_t>();
        HIP_TRY(launch_extract_count(a, c->stream));
        uint64_t total = 0;
        if (int rc = scan_total(a.part, blocks, c->stream, &total)) return rc;
        if (total == 0) break;
        if (a.leaf) { count = total; break; }
        if (total >= (uint64_t(1) << 32)) { set_error(std::string(who) + ": a tree level of 2^32 nodes or more"); return VXRT_E_INVALID; }
        if (hipError_t e = ensure(x.front[cur ^ 1], size_t(total) * sizeof(uint4)); e != hipSuccess)
            return alloc_failed(e, who, "the frontier");
        a.next = x.front[cur ^ 1].buf.as<uint4>();
        HIP_TRY(launch_extract_expand(a, c->stream));
        a.next = nullptr;
        cur ^= 1;
        frontier = uint32_t(total);
    }
    if (count_only || count == 0) { *n = size_t(count); return VXRT_OK; }
    if (cap < count) {
        *n = size_t(count);
        set_error(std::string(who) + ": " + std::to_string(count) + " voxels, room for " + std::to_string(cap));
        return VXRT_E_INVALID;
    }
    // the leaf parents' frontier is still in place (a.front, a.n, a.part): write the voxels at their offsets.  A device destination
    // is written in place where the kernel's stores fit its alignment (2 bytes per coordinate, 4 per mrgb word); otherwise, and for
    // the host, the voxels are staged in the context's buffers and copied out.
    const bool direct = device && (reinterpret_cast<uintptr_t>(pos) & 1u) == 0u && (reinterpret_cast<uintptr_t>(mrgb) & 3u) == 0u;
    if (direct) {
        a.pos = reinterpret_cast<int16_t*>(pos);
        a.mrgb = reinterpret_cast<uint32_t*>(mrgb);
    } else {
        if (hipError_t e = ensure(x.pos, size_t(count) * 3 * sizeof(int16_t)); e != hipSuccess) return alloc_failed(e, who, "the positions");
        if (hipError_t e = ensure(x.mrgb, size_t(count) * 4); e != hipSuccess) return alloc_failed(e, who, "the leaf words");
        a.pos = x.pos.buf.as<int16_t>();
        a.mrgb = x.mrgb.buf.as<uint32_t>();
    }
    HIP_TRY(launch_extract_expand(a, c->stream));
    if (!direct) {
        const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
        HIP_TRY(hipMemcpyAsync(pos, x.pos.buf, size_t(count) * 3 * sizeof(int16_t), kind, c->stream));
        HIP_TRY(hipMemcpyAsync(mrgb, x.mrgb.buf, size_t(count) * 4, kind, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n = size_t(count);
    return VXRT_OK;
}

}  // namespace vxrt

extern "C" {

int vxrt_get_voxels(vxrt_ctx* c, const int32_t box_min[3], const int32_t box_max[3], int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap,
                    size_t* n) try {
    return vxrt::get_voxels(c, box_min, box_max, pos, mrgb, cap, n, false, "vxrt_get_voxels");
} VXRT_CATCH

int vxrt_get_voxels_device(vxrt_ctx* c, const int32_t box_min[3], const int32_t box_max[3], int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap,
                           size_t* n) try {
    return vxrt::get_voxels(c, box_min, box_max, pos, mrgb, cap, n, true, "vxrt_get_voxels_device");
} VXRT_CATCH

}  // extern "C"
