// api_setops.hip — host side of vxrt_setops.h: two voxel lists in device memory combined under a set operation.  Each list is
// keyed, sorted and deduplicated by list_ops.h's key_list; the two sets go through its merge (setops.hip's kernel, counting and then
// emitting), and the result, which the merge leaves in path order, through its decode.  What is here are the op's rules: which
// arguments it needs and when B's bytes are carried.  Nothing but three counts and the lists' bounds crosses to the host.
// DESIGN.md §24.
#include <string>

#include "list_ops.h"
#include "scene_args.h"
#include "../../include/vxrt_setops.h"

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
    if (with_vals && b_bytes && nb != 0 && !b_mrgb) { set_error(w + ": this op takes bytes from B: null b_mrgb"); return VXRT_E_INVALID; }
    if (!with_vals && b_mrgb) { set_error(w + ": b_mrgb without a_mrgb"); return VXRT_E_INVALID; }
    if (int rc = check_output_pair(with_vals, out_pos, out_mrgb, who, "a_mrgb")) return rc;
    if (!with_vals && op == VXRT_LIST_CHANGED) { set_error(w + ": VXRT_LIST_CHANGED compares bytes: null a_mrgb"); return VXRT_E_INVALID; }
    if ((na != 0 && !a_pos) || (nb != 0 && !b_pos)) { set_error(w + ": null voxel positions"); return VXRT_E_INVALID; }
    if (na == 0 && nb == 0) { *n_out = 0; return VXRT_OK; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_input_list(c, a_pos, a_mrgb, na, who, "a_pos", "a_mrgb")) return rc;
    if (int rc = check_input_list(c, b_pos, b_mrgb, nb, who, "b_pos", "b_mrgb")) return rc;
    if (int rc = check_output_arrays(c, out_pos, out_mrgb, cap, who)) return rc;

    // both lists: sorted, one key per position, the last entry's bytes.  Every input byte is read here, into scratch, before the
    // decode at the end writes the first output byte.
    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    // A counting call carries the leaf words through the sort only where the count depends on them (CHANGED).
    const bool front_vals = with_vals && (out_pos != nullptr || op == VXRT_LIST_CHANGED);
    KeyedList fa, fb;
    if (int rc = key_list(a_pos, a_mrgb, na, front_vals, s, who, &fa, nullptr)) return rc;
    if (int rc = key_list(b_pos, b_mrgb, nb, front_vals && b_bytes, s, who, &fb, nullptr)) return rc;      // otherwise B is a mask
    if (uint64_t(fa.view.m) + uint64_t(fb.view.m) >= (uint64_t(1) << 32)) {
        set_error(w + ": 2^32 distinct positions or more in the two lists");
        return VXRT_E_INVALID;
    }

    // the result: (key, leaf word) per kept item at the scanned offsets, ascending and unique as the merge leaves it, decoded
    SetMerge mg;
    if (int rc = merge_count(fa.view, fb.view, op, s, who, &mg)) return rc;
    if (int rc = list_room(mg.count, out_pos, cap, who, n_out)) return rc;
    if (!out_pos || mg.count == 0) return VXRT_OK;
    OwnedSet out;
    if (int rc = merge_emit(&mg, s, who, "the result's", &out)) return rc;
    return decode_list(out.view.keys, out.view.words, mg.count, out_pos, out_mrgb, s);
} VXRT_CATCH

}  // extern "C"
