// api_morph.hip — host side of vxrt_morph.h: a voxel list in device memory dilated, eroded, or cut down to its surface layer or its
// margin ring.  The list is keyed, sorted and deduplicated by list_ops.h's key_list, once per call; every step then works on unique
// ascending keys and their leaf words.  morph.hip gives each voxel its neighbour mask; ERODE compacts by it, DILATE lets the voxels
// beside empty cells offer themselves, sorts the offers (a KeySort), keeps each cell's first (list_ops.h's run heads) and merges
// the new cells in (list_ops.h's merge); SURFACE and MARGIN end in that merge's DIFFERENCE against the original set; the totals, the output
// checks and the decode are list_ops.h's too.  What is here are the two steps and the loop over them.  Nothing but counts crosses
// to the host.  DESIGN.md §25.
#include <string>

#include "list_ops.h"
#include "morph.h"
#include "scene_args.h"
#include "../../include/vxrt_morph.h"

namespace vxrt {
namespace {

// The merge over two sets (b.m may be 0: b.keys is readable all the same; b.words == nullptr: b is a mask) -> *out, exactly sized;
// an empty result leaves out->view.m == 0 and allocates nothing.  Launches: the counting merge, the scan, the emitting merge.  Waits.
int merge_sets(const MorphSet& a, const MorphSet& b, uint32_t op, hipStream_t s, const char* who, OwnedSet* out) {
    if (uint64_t(a.m) + uint64_t(b.m) >= (uint64_t(1) << 32)) {
        set_error(std::string(who) + ": a step's result has 2^32 voxels or more");
        return VXRT_E_INVALID;
    }
    SetMerge mg;
    if (int rc = merge_count(a, b, op, s, who, &mg)) return rc;
    out->view = MorphSet{nullptr, nullptr, 0u};
    if (mg.count == 0) return VXRT_OK;
    if (int rc = merge_emit(&mg, s, who, "a step's", out)) return rc;
    HIP_TRY(hipStreamSynchronize(s));      // mg.part is freed on return
    return VXRT_OK;
}

// One step of ERODE on `in` (in.m > 0) -> *out; an empty result leaves out->view.m == 0.  Launches: the mask, the scan, the write.
int erode_step(const MorphSet& in, uint32_t c, bool tile, bool with_vals, hipStream_t s, const char* who, OwnedSet* out) {
    const uint32_t blocks = morph_blocks(in.m);
    ScratchBuffer masks, part;
    if (int rc = alloc_scratch(&masks, size_t(in.m) * sizeof(uint32_t), who, "the neighbour masks")) return rc;
    if (int rc = alloc_part(&part, in.m, who)) return rc;
    HIP_TRY(launch_morph_mask(in, c, kMorphErode, tile, masks.as<uint32_t>(), part.as<uint64_t>(), s));
    uint64_t count = 0;
    if (int rc = scan_total(part.as<uint64_t>(), blocks, s, &count)) return rc;
    out->view = MorphSet{nullptr, nullptr, 0u};
    if (count == 0) return VXRT_OK;
    if (int rc = alloc_set(out, count, with_vals, who, "a step's")) return rc;
    HIP_TRY(launch_morph_keep(in, c, masks.as<uint32_t>(), part.as<uint64_t>(), out->keys.as<uint64_t>(),
                              with_vals ? out->words.as<uint32_t>() : nullptr, s));
    HIP_TRY(hipStreamSynchronize(s));      // masks and part are freed on return
    return VXRT_OK;
}

// One step of DILATE on `in` (in.m > 0) -> *out.  Launches: the mask, the scan, the offers, the sort's 21 (7 digits of the 53
// bits), the first offers counted, the scan, the first offers written, and merge_sets' three.
int dilate_step(const MorphSet& in, uint32_t c, bool tile, bool with_vals, hipStream_t s, const char* who, OwnedSet* out) {
    const std::string w = who;
    const uint32_t blocks = morph_blocks(in.m);
    ScratchBuffer masks, part;
    if (int rc = alloc_scratch(&masks, size_t(in.m) * sizeof(uint32_t), who, "the neighbour masks")) return rc;
    if (int rc = alloc_part(&part, in.m, who)) return rc;
    HIP_TRY(launch_morph_mask(in, c, kMorphDilate, tile, masks.as<uint32_t>(), part.as<uint64_t>(), s));
    uint64_t offers = 0;
    if (int rc = scan_total(part.as<uint64_t>(), blocks, s, &offers)) return rc;
    if (offers >= (uint64_t(1) << 32)) { set_error(w + ": a step has 2^32 candidates or more"); return VXRT_E_INVALID; }
    if (offers == 0) { set_error(w + ": internal error: a set without an empty cell beside it"); return VXRT_E_INVALID; }

    // the offers, sorted by (cell, row as the cell sees the source): the first of each cell is its first source
    KeySort sort;
    if (int rc = sort.alloc(size_t(offers), with_vals, who)) return rc;
    HIP_TRY(launch_morph_offer(in, c, masks.as<uint32_t>(), part.as<uint64_t>(), sort.keys(), sort.vals(), s));
    HIP_TRY(sort.sort(uint32_t(offers), 53u, s));
    RunHeads firsts;      // freed on return, behind merge_sets' wait
    OwnedSet cells;
    if (int rc = run_heads(sort.keys(), sort.vals(), uint32_t(offers), kMorphOfferShift, with_vals, s, who, "a step's", &firsts, &cells)) return rc;
    // the new cells and the set are disjoint: UNION interleaves them
    return merge_sets(in, cells.view, kListUnion, s, who, out);
}

}  // namespace
}  // namespace vxrt

extern "C" {

int vxrt_morph_voxels_device(vxrt_ctx* c, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, uint32_t op, uint32_t connectivity,
                             uint32_t steps, int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], size_t cap, size_t* n_out) try {
    using namespace vxrt;
    const char* who = "vxrt_morph_voxels_device";
    const std::string w = who;
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error(w + ": 2^32 voxels or more"); return VXRT_E_INVALID; }
    if (!n_out) { set_error(w + ": null n_out"); return VXRT_E_INVALID; }
    if (op > uint32_t(VXRT_MORPH_MARGIN)) { set_error(w + ": op is no vxrt_morph_op"); return VXRT_E_INVALID; }
    if (connectivity != 6u && connectivity != 18u && connectivity != 26u) { set_error(w + ": connectivity must be 6, 18 or 26"); return VXRT_E_INVALID; }
    if (steps < 1u || steps > kMorphMaxSteps) { set_error(w + ": steps must lie in 1 .. 64"); return VXRT_E_INVALID; }
    const bool with_vals = mrgb != nullptr;
    if (int rc = check_output_pair(with_vals, out_pos, out_mrgb, who, "mrgb")) return rc;
    if (n != 0 && !pos) { set_error(w + ": null voxel positions"); return VXRT_E_INVALID; }
    if (n == 0) { *n_out = 0; return VXRT_OK; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_input_list(c, pos, mrgb, n, who, "pos", "mrgb")) return rc;
    if (int rc = check_output_arrays(c, out_pos, out_mrgb, cap, who)) return rc;

    // the list: sorted, one key per position, the last entry's bytes.  Every input byte is read here, into scratch, before the
    // decode at the end writes the first output byte.  A counting call leaves the leaf words behind: no count depends on them.
    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    const bool vals = with_vals && out_pos != nullptr;
    KeyedList list;
    if (int rc = key_list(pos, mrgb, n, vals, s, who, &list, nullptr)) return rc;
    const MorphSet original = list.view;      // 0 < m <= n

    // the steps, each on the result of the one before; an eroded set that is empty stays empty
    const bool grow = op == VXRT_MORPH_DILATE || op == VXRT_MORPH_MARGIN;
    const bool tile = c->morph_tile_lookup != 0;      // off in the product: the plain lookup measured faster (vxrt_debug.h has the switch)
    OwnedSet now;
    now.view = original;
    for (uint32_t step = 0; step < steps && now.view.m != 0u; step++) {
        OwnedSet next;
        if (int rc = grow ? dilate_step(now.view, connectivity, tile, vals, s, who, &next) : erode_step(now.view, connectivity, tile, vals, s, who, &next)) return rc;
        now.take(&next);      // the set before goes with `next`
    }
    if (op == VXRT_MORPH_SURFACE || op == VXRT_MORPH_MARGIN) {
        ScratchBuffer none;      // an empty set's keys: readable, never used
        if (int rc = alloc_scratch(&none, 0, who, "the keys")) return rc;
        MorphSet mask = grow ? original : now.view;
        if (mask.m == 0u) mask.keys = none.as<uint64_t>();
        mask.words = nullptr;      // DIFFERENCE takes b as a mask
        OwnedSet cut;
        if (int rc = merge_sets(grow ? now.view : original, mask, kListDifference, s, who, &cut)) return rc;
        now.take(&cut);
    }

    if (int rc = list_room(now.view.m, out_pos, cap, who, n_out)) return rc;
    if (!out_pos || now.view.m == 0u) return VXRT_OK;
    return decode_list(now.view.keys, now.view.words, now.view.m, out_pos, out_mrgb, s);
} VXRT_CATCH

int vxrt_debug_morph_tile_lookup(vxrt_ctx* c, uint32_t enable) try {
    if (!vxrt::valid_ctx(c)) { vxrt::set_error("null context"); return VXRT_E_INVALID; }
    c->morph_tile_lookup = enable != 0u ? 1 : 0;
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
