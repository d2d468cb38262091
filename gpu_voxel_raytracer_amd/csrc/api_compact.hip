// api_compact.hip — host side of vxrt_compact.h: the live tree of an edited scene written into new arrays in the layout of a fresh
// build (compact.hip), then swapped in, and the storage counts a host decides by.  The host runs the levels (compact.h) and reads
// back one number per level, the size of the next; the old arrays stay untouched until every level is written.  DESIGN.md §16.
#include <string>

#include "../../include/vxrt_compact.h"
#include "compact.h"
#include "ctx.h"
#include "device_build.h"
#include "list_ops.h"
#include "scene_args.h"

namespace vxrt {
namespace {

constexpr const char* kWho = "vxrt_compact_scene";

int miscounted(uint64_t found, size_t live) {
    set_error(std::string(kWho) + ": " + std::to_string(found) + " records reached from the root, " + std::to_string(live) + " counted");
    return VXRT_E_SCENE;
}

// The context's tree in new arrays (exactly sized; the caller's on VXRT_OK): *svo with c->live_nodes records, *leaves with
// *leaf_count words.  The context is drained and is not changed; nothing is left allocated on failure.
int relayout(vxrt_ctx* c, DeviceBuf<SvoRecord>* svo, DeviceBuf<int32_t>* leaves, size_t* leaf_count) {
    const size_t live = c->live_nodes;
    const uint32_t L = c->depth;
    if (live == 0 || live > c->svo_count) return miscounted(0, live);
    if (hipError_t e = svo->alloc(live); e != hipSuccess) return alloc_failed(e, kWho, "the records");
    if ((c->root_rec.masks & 0xffffu) == 0u) {
        // an empty scene: what upload_svo gives an empty list (flatten_svo: the root {0, 1}, and one zero leaf word)
        if (live != 1) return miscounted(1, live);
        if (hipError_t e = leaves->alloc(1); e != hipSuccess) return alloc_failed(e, kWho, "the leaf words");
        const SvoRecord root{0u, 1u};
        HIP_TRY(hipMemcpyAsync(svo->get(), &root, sizeof root, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemsetAsync(leaves->get(), 0, sizeof(int32_t), c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        *leaf_count = 1;
        return VXRT_OK;
    }
    ScratchBuffer part;
    if (int rc = alloc_scratch(&part, (size_t(compact_blocks(1, uint32_t(live))) + 1) * sizeof(uint64_t), kWho, "the scan partials")) return rc;
    CompactLevel a{};
    a.src = c->d_svo;
    a.src_leaves = c->d_leaves;
    a.src_count = uint32_t(c->svo_count);
    a.src_leaf_count = uint32_t(c->leaf_count);
    a.dst = svo->get();
    a.dst_count = uint32_t(live);
    a.part = part.as<uint64_t>();
    HIP_TRY(hipMemsetAsync(a.dst, 0, sizeof(SvoRecord), c->stream));   // the root: {0, old record 0}
    uint64_t start = 0, n = 1;
    for (uint32_t l = 0; l <= L; l++) {
        a.start = uint32_t(start);
        a.n = uint32_t(n);
        a.leaf = l == L ? 1u : 0u;
        const uint32_t blocks = compact_blocks(a.start, a.n);
        HIP_TRY(launch_compact_count(a, c->stream));
        uint64_t total = 0;
        if (int rc = scan_total(a.part, blocks, c->stream, &total)) return rc;
        if (a.leaf) {
            if (start + n != live) return miscounted(start + n, live);
            if (total == 0 || total > c->leaf_count) { set_error(std::string(kWho) + ": the leaf parents hold " + std::to_string(total) + " leaf words"); return VXRT_E_SCENE; }
            if (hipError_t e = leaves->alloc(size_t(total)); e != hipSuccess) return alloc_failed(e, kWho, "the leaf words");
            a.dst_leaves = leaves->get();
            a.dst_leaf_count = uint32_t(total);
            *leaf_count = size_t(total);
        } else if (total == 0 || start + n + total > live) {
            return miscounted(start + n + total, live);   // a level without nodes above the leaf parents, or more nodes than counted
        }
        HIP_TRY(launch_compact_expand(a, c->stream));
        start += n;
        n = total;
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VXRT_OK;
}

}  // namespace
}  // namespace vxrt

extern "C" {

int vxrt_compact_scene(vxrt_ctx* c) try {
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (int rc = require_scene(c)) return rc;
    if (int rc = require_editable_scene(c)) return rc;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = sync_all(c)) return rc;   // frames enqueued before the call read the old arrays
    if (!c->edited && c->svo_cap == 0 && c->leaf_cap == 0) return VXRT_OK;   // as built: breadth first, tight, exactly sized
    DeviceBuf<SvoRecord> svo;
    DeviceBuf<int32_t> leaves;
    size_t leaf_count = 0;
    if (int rc = relayout(c, &svo, &leaves, &leaf_count)) return rc;
    const SvoRecord root{c->root_rec.masks, (c->root_rec.masks & 0xffffu) == 0u || c->depth != 0 ? 1u : 0u};   // the new record 0
    bool box_valid = false;
    float box_min[3] = {0, 0, 0}, box_max[3] = {0, 0, 0};
    if (int rc = device_scene_box(svo, c->live_nodes, c->depth, root, c->root_center, c->root_size, &box_valid, box_min, box_max))
        return rc;
    // from here on the change happens: the new arrays replace the old, with a fresh scene's bookkeeping
    replace_scene_arrays(c, std::move(svo), c->live_nodes, std::move(leaves), leaf_count, {}, 0);
    c->root_rec = root;
    scene_replaced(c);
    c->box_valid = box_valid;
    for (int ax = 0; ax < 3; ax++) { c->box_min[ax] = box_min[ax]; c->box_max[ax] = box_max[ax]; }
    return VXRT_OK;
} VXRT_CATCH

int vxrt_get_scene_storage(vxrt_ctx* c, vxrt_scene_storage* out) try {
    if (!valid_ctx(c) || !out) { set_error("null argument"); return VXRT_E_INVALID; }
    if (int rc = require_scene(c)) return rc;
    out->records_live = c->live_nodes;
    out->records_used = c->svo_count;
    out->records_capacity = c->svo_cap ? c->svo_cap : c->svo_count;
    out->leaves_used = c->leaf_count;
    out->leaves_capacity = c->leaf_cap ? c->leaf_cap : c->leaf_count;
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
