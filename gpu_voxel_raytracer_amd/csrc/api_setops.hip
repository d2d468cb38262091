// api_setops.hip — host side of vxrt_setops.h: two voxel lists in device memory combined under a set operation.  Each list is keyed
// at depth 15 by the device editor's pass (device_edit.hip) and sorted and deduplicated by the list builder's front (device_build.h:
// sort_unique_list); the two key arrays are merged by setops.hip, the blocks' counts are summed by the list builder's scan and the
// result, which the merge leaves in path order, is decoded by transform.hip's decode.  Nothing but three counts and the lists'
// bounds crosses to the host.  DESIGN.md §24.
#include <string>

#include "ctx.h"
#include "device_build.h"
#include "edit.h"
#include "scene_args.h"
#include "setops.h"
#include "transform.h"
#include "../../include/vxrt_setops.h"

namespace vxrt {
namespace {

// One list through the front: m unique ascending keys in keys(), their leaf words in words() (nullptr without values).  An empty
// list gets the 16 readable bytes of alloc_scratch per array, which the merge's clamped loads may touch and never use.
struct FrontList {
    ListScratch ls;
    ScratchBuffer leaves;
    size_t m = 0;
    int cur = 0;
    bool with_vals = false;
    const uint64_t* keys() const { return ls.keys[cur].as<uint64_t>(); }
    const uint32_t* words() const { return with_vals ? leaves.as<uint32_t>() : nullptr; }
};

int run_front(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, bool with_vals, hipStream_t s, const char* who, FrontList* f) {
    f->with_vals = with_vals;
    if (n == 0) {
        if (int rc = alloc_scratch(&f->ls.keys[0], 0, who, "the keys")) return rc;
        return with_vals ? alloc_scratch(&f->leaves, 0, who, "the leaf words") : VXRT_OK;
    }
    if (int rc = alloc_list_scratch(n, with_vals, who, &f->ls)) return rc;
    ListBounds lb;
    if (int rc = edit_keys_device(reinterpret_cast<const int16_t*>(pos), with_vals ? reinterpret_cast<const uint8_t*>(mrgb) : nullptr, n, 15u,
                                  f->ls.keys[0].as<uint64_t>(), with_vals ? f->ls.vals[0].as<uint32_t>() : nullptr, s, who, &lb))
        return rc;
    return sort_unique_list(&f->ls, uint32_t(n), 15u, &f->leaves, s, who, &f->m, &f->cur);
}

}  // namespace
}  // namespace vxrt

extern "C" {

int vxrt_combine_voxels_device(vxrt_ctx* c, const int16_t (*a_pos)[3], const uint8_t (*a_mrgb)[4], size_t na, const int16_t (*b_pos)[3],
                               const uint8_t (*b_mrgb)[4], size_t nb, uint32_t op, int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], size_t cap,
                               size_t* n_out) try {
    using namespace vxrt;
    const char* who = "vxrt_combine_voxels_device";
    const std::string w = who;
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (uint64_t(na) >= (uint64_t(1) << 32) || uint64_t(nb) >= (uint64_t(1) << 32)) {
        set_error(w + ": 2^32 voxels or more in a list");
        return VXRT_E_INVALID;
    }
    if (!n_out) { set_error(w + ": null n_out"); return VXRT_E_INVALID; }
    if (op > uint32_t(VXRT_LIST_CHANGED)) { set_error(w + ": op is no vxrt_list_op"); return VXRT_E_INVALID; }
    const bool with_vals = a_mrgb != nullptr;
    const bool b_bytes = op == VXRT_LIST_UNION || op == VXRT_LIST_XOR || op == VXRT_LIST_CHANGED;    // the ops that keep items of B
    if (with_vals) {
        if (b_bytes && nb != 0 && !b_mrgb) { set_error(w + ": this op takes bytes from B: null b_mrgb"); return VXRT_E_INVALID; }
        if ((out_pos != nullptr) != (out_mrgb != nullptr)) { set_error(w + ": out_pos and out_mrgb come both or neither"); return VXRT_E_INVALID; }
    } else {
        if (b_mrgb) { set_error(w + ": b_mrgb without a_mrgb"); return VXRT_E_INVALID; }
        if (out_mrgb) { set_error(w + ": out_mrgb without a_mrgb"); return VXRT_E_INVALID; }
        if (op == VXRT_LIST_CHANGED) { set_error(w + ": VXRT_LIST_CHANGED compares bytes: null a_mrgb"); return VXRT_E_INVALID; }
    }
    if ((na != 0 && !a_pos) || (nb != 0 && !b_pos)) { set_error(w + ": null voxel positions"); return VXRT_E_INVALID; }
    if (na == 0 && nb == 0) { *n_out = 0; return VXRT_OK; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (na != 0) {
        if (int rc = check_device_array(c, a_pos, na * 3 * sizeof(int16_t), who, "a_pos")) return rc;
        if (a_mrgb)
            if (int rc = check_device_array(c, a_mrgb, na * 4, who, "a_mrgb")) return rc;
    }
    if (nb != 0) {
        if (int rc = check_device_array(c, b_pos, nb * 3 * sizeof(int16_t), who, "b_pos")) return rc;
        if (b_mrgb)
            if (int rc = check_device_array(c, b_mrgb, nb * 4, who, "b_mrgb")) return rc;
    }
    if (out_pos)
        if (int rc = check_device_array(c, out_pos, cap * 3 * sizeof(int16_t), who, "out_pos")) return rc;
    if (out_mrgb)
        if (int rc = check_device_array(c, out_mrgb, cap * 4, who, "out_mrgb")) return rc;

    // both lists: keys at depth 15 (every int16 position is inside that cube), sorted, one per position, the last entry's bytes.
    // Every input byte is read here, into scratch, before the decode at the end writes the first output byte.
    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    // A counting call carries the leaf words through the sort only where the count depends on them (CHANGED).
    const bool front_vals = with_vals && (out_pos != nullptr || op == VXRT_LIST_CHANGED);
    FrontList fa, fb;
    if (int rc = run_front(a_pos, a_mrgb, na, front_vals, s, who, &fa)) return rc;
    if (int rc = run_front(b_pos, b_mrgb, nb, front_vals && b_bytes, s, who, &fb)) return rc;      // otherwise B is a mask
    const uint64_t items = uint64_t(fa.m) + uint64_t(fb.m);
    if (items >= (uint64_t(1) << 32)) { set_error(w + ": 2^32 distinct positions or more in the two lists"); return VXRT_E_INVALID; }

    const uint32_t blocks = setop_blocks(items);
    ScratchBuffer part;
    if (int rc = alloc_scratch(&part, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    SetopArgs a{};
    a.keys_a = fa.keys();
    a.words_a = fa.words();
    a.keys_b = fb.keys();
    a.words_b = fb.words();
    a.ma = uint32_t(fa.m);
    a.mb = uint32_t(fb.m);
    a.op = op;
    a.part = part.as<uint64_t>();
    HIP_TRY(launch_setop_merge(a, s));
    HIP_TRY(launch_exclusive_scan(a.part, blocks, s));
    uint64_t count = 0;
    HIP_TRY(hipMemcpyAsync(&count, a.part + blocks, sizeof count, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_out = size_t(count);
    if (!out_pos || count == 0) return VXRT_OK;
    if (count > cap) {
        set_error(w + ": " + std::to_string(count) + " voxels, room for " + std::to_string(cap));
        return VXRT_E_INVALID;
    }

    // the result: (key, leaf word) per kept item at the scanned offsets, ascending and unique as the merge leaves it, decoded
    ScratchBuffer out_keys, out_words;
    if (int rc = alloc_scratch(&out_keys, size_t(count) * sizeof(uint64_t), who, "the result's keys")) return rc;
    if (front_vals)
        if (int rc = alloc_scratch(&out_words, size_t(count) * sizeof(uint32_t), who, "the result's leaf words")) return rc;
    a.out_keys = out_keys.as<uint64_t>();
    a.out_words = front_vals ? out_words.as<uint32_t>() : nullptr;
    HIP_TRY(launch_setop_merge(a, s));
    HIP_TRY(launch_transform_decode(a.out_keys, a.out_words, uint32_t(count), reinterpret_cast<uint8_t*>(out_pos), reinterpret_cast<uint8_t*>(out_mrgb), s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
