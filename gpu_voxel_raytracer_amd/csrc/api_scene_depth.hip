// api_scene_depth.hip — host side of vxrt_scene_depth.h: the octree depth of a loaded scene changed in place.  The host decides from
// the root record and, for a shrink or a fit, one probe of the paths below the root's children; the surgery is one launch of
// scene_depth.hip.  DESIGN.md §14.
#include "../../include/vxrt_scene_depth.h"
#include "ctx.h"
#include "edit.h"
#include "scene_args.h"

namespace vxrt {
namespace {

// the root's children (leaf words at depth 0)
uint32_t root_mask(const vxrt_ctx* c) { return c->depth == 0 ? (c->root_rec.masks >> 8) & 0xffu : c->root_rec.masks & 0xffu; }

// what the paths below the root allow (edit.h: launch_depth_probe): *levels the scene can lose, *one = it is the voxel (-2^t)^3
int probe_depth(vxrt_ctx* c, const char* who, uint32_t* levels, bool* one) {
    *levels = c->depth;
    *one = false;
    if (root_mask(c) == 0u) return VXRT_OK;   // empty: any depth holds it
    ScratchBuffer out;
    if (int rc = alloc_scratch(&out, 2 * sizeof(uint32_t), who, "the probe's result")) return rc;
    HIP_TRY(launch_depth_probe(c->d_svo, c->root_rec, c->depth, out.as<uint32_t>(), c->stream));
    uint32_t h[2];
    HIP_TRY(hipMemcpyAsync(h, out.get(), sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *levels = h[0];
    *one = h[1] != 0u;
    return VXRT_OK;
}

// The scene at depth `to` (arguments checked; a shrink was allowed by the probe; the context is drained).
int change_depth(vxrt_ctx* c, uint32_t to) {
    const uint32_t from = c->depth, M = root_mask(c), m = uint32_t(__builtin_popcount(M));
    if (to == from) return VXRT_OK;
    // storage: a grow adds the root's block and one 8-entry block per new node (edit.h: launch_depth_grow); a shrink to depth 0 the
    // root's leaf block
    size_t svo_add = 0, leaf_add = 0;
    if (M != 0u && to > from) {
        const size_t g = to - from;
        svo_add = 8 + 8 * size_t(m) * (from == 0 ? g - 1 : g);
        leaf_add = from == 0 ? 8 * size_t(m) : 0;
    } else if (M != 0u && to == 0) {
        leaf_add = 8;
    }
    GrownStorage grown;
    if (int rc = grow_storage(c, c->svo_count + svo_add, c->leaf_count + leaf_add, &grown)) return rc;
    // from here on the change happens
    commit_storage(c, std::move(grown));
    if (!c->edited) { c->edited = true; c->svo_built = c->svo_count; c->leaf_built = c->leaf_count; }   // as apply_edit_batch
    SvoRecord root = c->root_rec;
    if (M != 0u && to > from) {
        HIP_TRY(launch_depth_grow(c->d_svo, c->d_leaves, root, from, to - from, uint32_t(c->svo_count), uint32_t(c->leaf_count), c->stream));
        root = SvoRecord{M, uint32_t(c->svo_count)};
        c->live_nodes += size_t(m) * (to - from);
    } else if (M != 0u) {
        HIP_TRY(launch_depth_shrink(c->d_svo, c->d_leaves, root, from, from - to, uint32_t(c->leaf_count), c->stream));
        if (to == 0) root = SvoRecord{M << 8, uint32_t(c->leaf_count)};
        c->live_nodes -= size_t(m) * (from - to);
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->svo_count += svo_add;
    c->leaf_count += leaf_add;
    c->root_rec = root;
    c->depth = to;
    c->root_size = float(1u << to);
    drop_touch_maps(c);   // sized for the records before the change; the DDA prototype's grid is of the old tree
    return VXRT_OK;
}

// the checks both calls share, in vxrt_edit_voxels's order; then the context is drained (frames enqueued before see the old scene)
int begin(vxrt_ctx* c) {
    if (int rc = require_scene(c)) return rc;
    if (int rc = require_editable_scene(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    return sync_all(c);
}

}  // namespace
}  // namespace vxrt

extern "C" {

int vxrt_set_scene_depth(vxrt_ctx* c, uint32_t depth) try {
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (depth > 15) { set_error("octree depth > 15"); return VXRT_E_INVALID; }
    if (int rc = begin(c)) return rc;
    if (depth < c->depth) {
        uint32_t levels;
        bool one;
        if (int rc = probe_depth(c, "vxrt_set_scene_depth", &levels, &one)) return rc;
        if (c->depth - depth > levels) {
            set_error("a voxel lies outside the root cube [-" + std::to_string(1u << depth) + ", " + std::to_string(1u << depth) +
                      ")^3 of depth " + std::to_string(depth));
            return VXRT_E_SCENE;
        }
    }
    return change_depth(c, depth);
} VXRT_CATCH

int vxrt_fit_scene_depth(vxrt_ctx* c, uint32_t* depth) try {
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (int rc = begin(c)) return rc;
    uint32_t levels;
    bool one;
    if (int rc = probe_depth(c, "vxrt_fit_scene_depth", &levels, &one)) return rc;
    const uint32_t fit = c->depth - levels + (one ? 1u : 0u);   // scene_host.cpp: build_octree's rule
    if (fit > 15) { set_error("the scene is the one voxel (-32768, -32768, -32768): its depth rule gives 16"); return VXRT_E_SCENE; }
    if (int rc = change_depth(c, fit)) return rc;
    if (depth) *depth = fit;
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
