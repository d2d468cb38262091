// api_query.hip — host side of vxrt_query.h: voxel lookups and ray casts against the loaded scene with every array in device memory.
// The kernels are query.hip's; the per-block counts of the lookup are summed by the list builder's scan (device_build.h).  Nothing
// but the count crosses to the host.  DESIGN.md §22.
#include <cstring>
#include <string>

#include "ctx.h"
#include "device_build.h"
#include "query.h"
#include "scene_args.h"
#include "../../include/vxrt_query.h"

extern "C" {

int vxrt_lookup_voxels_device(vxrt_ctx* c, const int16_t (*pos)[3], size_t n, const int32_t offset[3], uint32_t* leaf,
                              size_t* n_present) try {
    using namespace vxrt;
    const char* who = "vxrt_lookup_voxels_device";
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error(std::string(who) + ": 2^32 positions or more"); return VXRT_E_INVALID; }
    if (n == 0) {
        if (n_present) *n_present = 0;
        return VXRT_OK;
    }
    if (!pos) { set_error(std::string(who) + ": null positions"); return VXRT_E_INVALID; }
    if (!leaf && !n_present) { set_error(std::string(who) + ": leaf and n_present are both null"); return VXRT_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(leaf) & 3u) != 0u) { set_error(std::string(who) + ": leaf must be 4-byte aligned"); return VXRT_E_INVALID; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_device_array(c, pos, n * 3 * sizeof(int16_t), who, "pos")) return rc;
    if (leaf)
        if (int rc = check_device_array(c, leaf, n * sizeof(uint32_t), who, "leaf")) return rc;
    if (!c->has_scene) { set_error("no scene set"); return VXRT_E_NOSCENE; }
    if (c->depth >= kQueryLevels) { set_error(std::string(who) + ": a scene deeper than 15"); return VXRT_E_SCENE; }

    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    if (c->svo_count == 0 || c->leaf_count == 0 || !c->d_svo || !c->d_leaves) {   // no record 0 or no leaf word 0: a scene without a voxel
        if (leaf) HIP_TRY(hipMemsetAsync(leaf, 0, n * sizeof(uint32_t), s));
        HIP_TRY(hipStreamSynchronize(s));
        if (n_present) *n_present = 0;
        return VXRT_OK;
    }
    const uint32_t blocks = query_blocks(n);
    ScratchBuffer part;
    if (n_present)
        if (int rc = alloc_scratch(&part, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    LookupArgs a{};
    a.svo = c->d_svo;
    a.leaves = c->d_leaves;
    a.root_rec = c->root_rec;
    a.depth = c->depth;
    if (offset) memcpy(a.offset, offset, sizeof a.offset);
    a.pos = reinterpret_cast<const int16_t*>(pos);
    a.n = uint32_t(n);
    a.leaf = leaf;
    a.part = part.as<uint64_t>();
    HIP_TRY(launch_query_lookup(a, s));
    uint64_t count = 0;
    if (n_present) {
        HIP_TRY(launch_exclusive_scan(a.part, blocks, s));
        HIP_TRY(hipMemcpyAsync(&count, a.part + blocks, sizeof count, hipMemcpyDeviceToHost, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    if (n_present) *n_present = size_t(count);
    return VXRT_OK;
} VXRT_CATCH

int vxrt_pick_device(vxrt_ctx* c, const float (*origins)[3], const float (*dirs)[3], const float* max_time, size_t n,
                     vxrt_pick_hit* out) try {
    using namespace vxrt;
    const char* who = "vxrt_pick_device";
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 31)) { set_error(std::string(who) + ": too many rays"); return VXRT_E_INVALID; }
    if (n == 0) return VXRT_OK;
    if (!origins || !dirs || !out) { set_error(std::string(who) + ": null argument"); return VXRT_E_INVALID; }
    const struct { const void* p; const char* what; size_t bytes; } arrays[] = {
        {max_time, "max_time", n * sizeof(float)}, {origins, "origins", n * 12}, {dirs, "dirs", n * 12}, {out, "out", n * sizeof(vxrt_pick_hit)}};
    for (const auto& v : arrays)
        if ((reinterpret_cast<uintptr_t>(v.p) & 3u) != 0u) { set_error(std::string(who) + ": " + v.what + " must be 4-byte aligned"); return VXRT_E_INVALID; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    for (const auto& v : arrays)
        if (v.p)
            if (int rc = check_device_array(c, v.p, v.bytes, who, v.what)) return rc;
    if (!c->has_scene) { set_error("no scene set"); return VXRT_E_NOSCENE; }

    HIP_TRY(launch_query_pick(pick_args(c), reinterpret_cast<const float*>(origins), reinterpret_cast<const float*>(dirs), max_time, out, unsigned(n), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
