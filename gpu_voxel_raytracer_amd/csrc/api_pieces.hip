// api_pieces.hip — host side of vxrt_pieces.h: the table of a voxel list's connected components (size, bounding box, coordinate sums,
// number) and the detached pieces of the loaded scene, and with them the bodies of vxrt_components.h's two calls, which ask for less
// of the same (pieces.h).  The labelling is api_components.hip's (components.h: label_list); what follows it is pieces.hip plus the
// scatter and selection kernels of components.hip.  Nothing but counts crosses to the host: the labelling's two, and for the scene
// calls the scene's, the selected voxels and the selected pieces.  DESIGN.md §20, §21.
#include <algorithm>
#include <string>

#include "pieces.h"
#include "scene_args.h"
#include "../../include/vxrt_device_edit.h"

namespace vxrt {
namespace {

// The accumulators of l's components, reduced: l->parent becomes the roots' slots (the labelling is done with its forest).
int reduce_pieces(Labelling* l, uint32_t anchored, const char* who, ScratchBuffer* accs, hipStream_t s) {
    if (int rc = alloc_scratch(accs, size_t(l->components) * sizeof(PieceAcc), who, "the components' accumulators")) return rc;
    HIP_TRY(pieces_slots(l->comp.as<uint32_t>(), l->acc.as<uint32_t>(), l->unique, l->part.as<uint64_t>(), anchored, l->parent.as<uint32_t>(),
                         accs->as<PieceAcc>(), s));
    HIP_TRY(pieces_reduce(l->ukeys, l->uhead.as<uint32_t>(), l->comp.as<uint32_t>(), l->parent.as<uint32_t>(), l->unique, accs->as<PieceAcc>(), s));
    return VXRT_OK;
}

// The selected components marked at their labels, in l->uhead (the reduce was its last reader), zeroed first.
int mark_pieces(Labelling* l, uint32_t n, uint32_t min_voxels, uint32_t max_voxels, PieceAcc* accs, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(l->uhead.get(), 0, size_t(n) * sizeof(uint32_t), s));
    HIP_TRY(pieces_mark(accs, uint32_t(l->components), n, min_voxels, max_voxels, l->uhead.as<uint32_t>(), s));
    return VXRT_OK;
}

size_t table_bytes(size_t entries, uint64_t at_most) { return size_t(std::min<uint64_t>(entries, at_most)) * sizeof(vxrt_piece); }

// The loaded scene's voxel list, in path order, into scratch: counted, then decoded (vxrt_get_voxels_device).  *total == 0: no list.
int scene_list(vxrt_ctx* c, const char* who, ScratchBuffer* pos, ScratchBuffer* mrgb, size_t* total) {
    if (int rc = vxrt_get_voxels_device(c, nullptr, nullptr, nullptr, nullptr, 0, total)) return rc;
    if (*total == 0) return VXRT_OK;
    if (int rc = alloc_scratch(pos, *total * 3 * sizeof(int16_t), who, "the scene's positions")) return rc;
    if (int rc = alloc_scratch(mrgb, *total * 4, who, "the scene's mrgb words")) return rc;
    size_t got = 0;
    return vxrt_get_voxels_device(c, nullptr, nullptr, reinterpret_cast<int16_t(*)[3]>(pos->get()), reinterpret_cast<uint8_t(*)[4]>(mrgb->get()), *total, &got);
}

}  // namespace

int component_table(const char* who, vxrt_ctx* c, const int16_t (*pos)[3], size_t n, uint32_t connectivity, uint32_t* label, uint32_t* id,
                    vxrt_piece* info, size_t info_cap, size_t* n_components) {
    if (!valid_ctx(c) || !n_components) { set_error("null argument"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error(std::string(who) + ": 2^32 voxels or more"); return VXRT_E_INVALID; }
    const uint32_t axes = axes_of(connectivity);
    if (axes == 0u) { set_error(std::string(who) + ": connectivity " + std::to_string(connectivity) + " (6, 18 or 26)"); return VXRT_E_INVALID; }
    if (n == 0) { *n_components = 0; return VXRT_OK; }
    if (!pos) { set_error(std::string(who) + ": null voxel positions"); return VXRT_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(label) & 3u) != 0u) { set_error(std::string(who) + ": label must be 4-byte aligned"); return VXRT_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(id) & 3u) != 0u) { set_error(std::string(who) + ": id must be 4-byte aligned"); return VXRT_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(info) & 7u) != 0u) { set_error(std::string(who) + ": info must be 8-byte aligned"); return VXRT_E_INVALID; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_device_array(c, pos, n * 3 * sizeof(int16_t), who, "pos")) return rc;
    if (label)
        if (int rc = check_device_array(c, label, n * sizeof(uint32_t), who, "label")) return rc;
    if (id)
        if (int rc = check_device_array(c, id, n * sizeof(uint32_t), who, "id")) return rc;
    if (info && info_cap != 0)      // a list of n entries has at most n components
        if (int rc = check_device_array(c, info, table_bytes(info_cap, n), who, "info")) return rc;

    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    const uint32_t nn = uint32_t(n);
    Labelling l;
    if (int rc = alloc_labelling(n, who, &l)) return rc;
    CompBox box{};
    if (int rc = label_list(reinterpret_cast<const int16_t*>(pos), nn, axes, box, s, &l)) return rc;
    *n_components = size_t(l.components);
    if (info && l.components > info_cap) {
        set_error(std::string(who) + ": " + std::to_string(l.components) + " components, room for " + std::to_string(info_cap));
        return VXRT_E_INVALID;
    }
    if (!id && !info) {            // labels only (vxrt_label_components_device asks for no more): no accumulators
        if (label) {
            HIP_TRY(components_scatter(l.sorted, l.rank, nn, l.comp.as<uint32_t>(), l.acc.as<uint32_t>(), 0u, label, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        return VXRT_OK;
    }
    ScratchBuffer accs;
    if (int rc = reduce_pieces(&l, 0u, who, &accs, s)) return rc;
    PieceAcc* pa = accs.as<PieceAcc>();
    if (int rc = mark_pieces(&l, nn, 0u, 0xffffffffu, pa, s)) return rc;      // every component
    const uint32_t* mark = l.uhead.as<uint32_t>();
    uint64_t* part = l.part.as<uint64_t>();      // the slots have read the root counts
    HIP_TRY(components_select_count(mark, nn, part, s));
    HIP_TRY(launch_exclusive_scan(part, comp_blocks(nn), s));
    HIP_TRY(pieces_number(mark, nn, part, nullptr, nullptr, pa, s));
    if (info) HIP_TRY(pieces_emit(pa, uint32_t(l.components), 0u, info, s));
    HIP_TRY(pieces_scatter(l.sorted, l.rank, nn, l.comp.as<uint32_t>(), l.parent.as<uint32_t>(), pa, label, id, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

int detached_pieces(const char* who, vxrt_ctx* c, const int32_t anchor_min[3], const int32_t anchor_max[3], uint32_t connectivity,
                    uint32_t min_voxels, uint32_t max_voxels, int16_t (*pos)[3], uint8_t (*mrgb)[4], uint32_t* piece, size_t cap, size_t* n,
                    vxrt_piece* info, size_t info_cap, size_t* n_pieces) {
    if (!valid_ctx(c) || !n) { set_error("null argument"); return VXRT_E_INVALID; }
    if (!anchor_min || !anchor_max) { set_error(std::string(who) + ": null anchor box"); return VXRT_E_INVALID; }
    const uint32_t axes = axes_of(connectivity);
    if (axes == 0u) { set_error(std::string(who) + ": connectivity " + std::to_string(connectivity) + " (6, 18 or 26)"); return VXRT_E_INVALID; }
    if ((pos == nullptr) != (mrgb == nullptr)) { set_error("pos and mrgb: both or neither"); return VXRT_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(piece) & 3u) != 0u) { set_error(std::string(who) + ": piece must be 4-byte aligned"); return VXRT_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(info) & 7u) != 0u) { set_error(std::string(who) + ": info must be 8-byte aligned"); return VXRT_E_INVALID; }
    if (int rc = require_scene(c)) return rc;
    const bool count_only = !pos && !piece && !info;
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (cap != 0) {
        if (pos) {
            if (int rc = check_device_array(c, pos, cap * 3 * sizeof(int16_t), who, "pos")) return rc;
            if (int rc = check_device_array(c, mrgb, cap * 4, who, "mrgb")) return rc;
        }
        if (piece)
            if (int rc = check_device_array(c, piece, cap * sizeof(uint32_t), who, "piece")) return rc;
    }
    if (info && info_cap != 0)      // a scene holds fewer than 2^32 voxels, so fewer pieces
        if (int rc = check_device_array(c, info, table_bytes(info_cap, uint64_t(1) << 32), who, "info")) return rc;

    size_t total = 0;
    ScratchBuffer spos, smrgb, flags, mark_part, accs;
    if (int rc = scene_list(c, who, &spos, &smrgb, &total)) return rc;
    if (total == 0) {
        *n = 0;
        if (n_pieces) *n_pieces = 0;
        return VXRT_OK;
    }
    const uint32_t nn = uint32_t(total);   // a scene holds fewer than 2^32 leaf words
    Labelling l;
    if (int rc = alloc_scratch(&flags, total * sizeof(uint32_t), who, "the flags")) return rc;
    if (n_pieces)
        if (int rc = alloc_scratch(&mark_part, (size_t(comp_blocks(total)) + 1) * sizeof(uint64_t), who, "the scan partials")) return rc;
    if (int rc = alloc_labelling(total, who, &l)) return rc;

    hipStream_t s = c->stream;
    CompBox box{};
    for (int ax = 0; ax < 3; ax++) { box.lo[ax] = anchor_min[ax]; box.hi[ax] = anchor_max[ax]; }
    box.on = 1u;
    if (int rc = label_list(spos.as<int16_t>(), nn, axes, box, s, &l)) return rc;
    // pick[i] != 0: entry i of the scene's list is returned
    uint32_t* pick = flags.as<uint32_t>();
    PieceAcc* pa = nullptr;
    const uint32_t* mark = nullptr;
    if (!n_pieces) {      // every detached voxel: the flatten's anchor marks decide, no accumulators
        HIP_TRY(components_scatter(l.sorted, l.rank, nn, l.comp.as<uint32_t>(), l.acc.as<uint32_t>(), 1u, pick, s));
    } else {              // the detached components within the size range
        if (int rc = reduce_pieces(&l, 1u, who, &accs, s)) return rc;
        pa = accs.as<PieceAcc>();
        if (int rc = mark_pieces(&l, nn, min_voxels, max_voxels, pa, s)) return rc;
        mark = l.uhead.as<uint32_t>();
        HIP_TRY(pieces_pick(l.sorted, l.rank, nn, l.comp.as<uint32_t>(), l.parent.as<uint32_t>(), pa, pick, s));
    }
    uint64_t* part = l.part.as<uint64_t>();      // the slots have read the root counts
    uint64_t count = 0, pieces = 0;
    HIP_TRY(components_select_count(pick, nn, part, s));
    HIP_TRY(launch_exclusive_scan(part, comp_blocks(nn), s));
    if (n_pieces) {
        HIP_TRY(components_select_count(mark, nn, mark_part.as<uint64_t>(), s));
        HIP_TRY(launch_exclusive_scan(mark_part.as<uint64_t>(), comp_blocks(nn), s));
    }
    HIP_TRY(hipMemcpyAsync(&count, part + comp_blocks(nn), sizeof count, hipMemcpyDeviceToHost, s));
    if (n_pieces) HIP_TRY(hipMemcpyAsync(&pieces, mark_part.as<uint64_t>() + comp_blocks(nn), sizeof pieces, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n = size_t(count);
    if (n_pieces) *n_pieces = size_t(pieces);
    if (count_only || count == 0) return VXRT_OK;
    if ((pos || piece) && cap < count) {
        set_error(std::string(who) + ": " + std::to_string(count) + " voxels, room for " + std::to_string(cap));
        return VXRT_E_INVALID;
    }
    if (info && info_cap < pieces) {
        set_error(std::string(who) + ": " + std::to_string(pieces) + " pieces, room for " + std::to_string(info_cap));
        return VXRT_E_INVALID;
    }
    if (n_pieces) HIP_TRY(pieces_number(mark, nn, mark_part.as<uint64_t>(), pick, part, pa, s));
    ScratchBuffer stage[2];
    if (pos)
        if (int rc = write_voxels_staged(pos, mrgb, size_t(count), s, who, stage, [&](int16_t* dst_pos, uint32_t* dst_mrgb) {
                return components_select_write(pick, nn, part, spos.as<int16_t>(), smrgb.as<uint32_t>(), dst_pos, dst_mrgb, s);
            }))
            return rc;
    if (piece) HIP_TRY(pieces_write(pick, nn, part, pa, piece, s));
    if (info) HIP_TRY(pieces_emit(pa, uint32_t(l.components), 1u, info, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

}  // namespace vxrt

extern "C" {

int vxrt_component_table_device(vxrt_ctx* c, const int16_t (*pos)[3], size_t n, uint32_t connectivity, uint32_t* label, uint32_t* id,
                                vxrt_piece* info, size_t info_cap, size_t* n_components) try {
    return vxrt::component_table("vxrt_component_table_device", c, pos, n, connectivity, label, id, info, info_cap, n_components);
} VXRT_CATCH

int vxrt_detached_pieces_device(vxrt_ctx* c, const int32_t anchor_min[3], const int32_t anchor_max[3], uint32_t connectivity, uint32_t min_voxels,
                                uint32_t max_voxels, int16_t (*pos)[3], uint8_t (*mrgb)[4], uint32_t* piece, size_t cap, size_t* n, vxrt_piece* info,
                                size_t info_cap, size_t* n_pieces) try {
    if (!n_pieces) { vxrt::set_error("null argument"); return VXRT_E_INVALID; }
    return vxrt::detached_pieces("vxrt_detached_pieces_device", c, anchor_min, anchor_max, connectivity, min_voxels, max_voxels, pos, mrgb, piece, cap,
                                 n, info, info_cap, n_pieces);
} VXRT_CATCH

}  // extern "C"
