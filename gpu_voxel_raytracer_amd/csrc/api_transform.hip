// api_transform.hip — host side of vxrt_transform.h: a voxel list in device memory resampled under a fixed-point affine map, by
// pulling every cell of a destination box through the map into the list.  The source is keyed, sorted and deduplicated by
// list_ops.h's key_list, which also gives its bounds; the pull is transform.hip's; the blocks' counts are summed by scan_total and
// the result is sorted by a KeySort (device_build.h); the output checks and the decode are list_ops.h's.
// Nothing but two counts and the source's bounds crosses to the host.  DESIGN.md §23.
#include <string>

#include "list_ops.h"
#include "scene_args.h"
#include "transform.h"
#include "../../include/vxrt_transform.h"

extern "C" {

int vxrt_transform_voxels_device(vxrt_ctx* c, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, const vxrt_affine* pull,
                                 const int32_t box_min[3], const int32_t box_max[3], int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4],
                                 size_t cap, size_t* n_out) try {
    using namespace vxrt;
    const char* who = "vxrt_transform_voxels_device";
    const std::string w = who;
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error(w + ": 2^32 voxels or more"); return VXRT_E_INVALID; }
    if (!pull || !n_out || !box_min || !box_max) { set_error(w + ": null argument"); return VXRT_E_INVALID; }
    if (pull->reserved != 0) { set_error(w + ": pull->reserved must be 0"); return VXRT_E_INVALID; }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++)
            if (pull->m[i][j] < -(int32_t(1) << 24) || pull->m[i][j] > (int32_t(1) << 24)) {
                set_error(w + ": an entry of pull->m beyond 2^24 (256.0 in Q16)");
                return VXRT_E_INVALID;
            }
        if (pull->t[i] < -(int64_t(1) << 40) || pull->t[i] > (int64_t(1) << 40)) {
            set_error(w + ": an entry of pull->t beyond 2^40 (2^24 cells in Q16)");
            return VXRT_E_INVALID;
        }
    }
    uint64_t cells = 1;
    bool empty_box = false;
    for (int ax = 0; ax < 3; ax++) {
        if (box_min[ax] < -32768 || box_min[ax] > 32768 || box_max[ax] < -32768 || box_max[ax] > 32768) {
            set_error(w + ": a box corner outside [-32768, 32768]");
            return VXRT_E_INVALID;
        }
        if (box_min[ax] >= box_max[ax]) empty_box = true;
        else cells *= uint64_t(box_max[ax] - box_min[ax]);      // each at most 2^16
    }
    if (!empty_box && cells >= (uint64_t(1) << 32)) { set_error(w + ": a box of 2^32 cells or more"); return VXRT_E_INVALID; }
    if (n != 0 && !pos) { set_error(w + ": null voxel positions"); return VXRT_E_INVALID; }
    if (int rc = check_output_pair(mrgb != nullptr, out_pos, out_mrgb, who, "mrgb")) return rc;
    if (empty_box || n == 0) { *n_out = 0; return VXRT_OK; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_input_list(c, pos, mrgb, n, who, "pos", "mrgb")) return rc;
    if (int rc = check_output_arrays(c, out_pos, out_mrgb, cap, who)) return rc;

    // the source: sorted, one key per position, the last entry's bytes (carried on a counting call too)
    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    const bool with_vals = mrgb != nullptr;
    const uint32_t blocks = pull_blocks(cells);
    KeyedList src;
    ScratchBuffer part;
    ListBounds lb;
    // allocated ahead of the front, whose last kernel is still running when it returns: the pull is enqueued right behind it
    if (int rc = alloc_scratch(&part, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    if (int rc = key_list(pos, mrgb, n, with_vals, s, who, &src, &lb)) return rc;

    PullArgs a{};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) a.m[i][j] = pull->m[i][j];
        a.t[i] = pull->t[i];
        a.lo[i] = box_min[i];
        a.ext[i] = uint32_t(box_max[i] - box_min[i]);
        a.src_lo[i] = lb.lo[i];
        a.src_hi[i] = lb.hi[i];
    }
    a.cells = uint32_t(cells);
    a.keys = src.view.keys;
    a.words = reinterpret_cast<const int32_t*>(src.view.words);
    a.count = src.view.m;      // 0 < m <= n
    a.part = part.as<uint64_t>();
    HIP_TRY(launch_transform_pull(a, s));
    uint64_t count = 0;
    if (int rc = scan_total(a.part, blocks, s, &count)) return rc;
    if (int rc = list_room(count, out_pos, cap, who, n_out)) return rc;
    if (!out_pos || count == 0) return VXRT_OK;

    // the result: (key of d, leaf word of s) per voxel at the scanned offsets, sorted by key (unique by construction), decoded
    KeySort out;
    if (int rc = out.alloc(size_t(count), with_vals, who)) return rc;
    a.out_keys = out.keys();
    a.out_words = out.vals();
    HIP_TRY(launch_transform_pull(a, s));
    HIP_TRY(out.sort(uint32_t(count), 48u, s));
    return decode_list(out.keys(), out.vals(), count, out_pos, out_mrgb, s);
} VXRT_CATCH

}  // extern "C"
