// api_morph.hip — host side of vxrt_morph.h: a voxel list in device memory dilated, eroded, or cut down to its surface layer or its
// margin ring.  The list is keyed at depth 15 by the device editor's pass (device_edit.hip) and sorted and deduplicated by the list
// builder's front (device_build.h: sort_unique_list), once per call; every step then works on unique ascending keys and their leaf
// words.  morph.hip gives each voxel its neighbour mask; ERODE compacts by it, DILATE lets the voxels beside empty cells offer
// themselves, sorts the offers (the list builder's radix sort), keeps each cell's first and merges the new cells in (setops.hip);
// SURFACE and MARGIN end in that merge's DIFFERENCE against the original set; transform.hip's decode writes the result.  Nothing
// but counts crosses to the host.  DESIGN.md §25.
#include <string>
#include <utility>

#include "ctx.h"
#include "device_build.h"
#include "edit.h"
#include "morph.h"
#include "scene_args.h"
#include "setops.h"
#include "transform.h"
#include "../../include/vxrt_morph.h"

namespace vxrt {
namespace {

// A set as the steps pass it on: unique ascending keys and, with values, their leaf words.  `view` is what the kernels read; the
// buffers own it, except for the first set, which is the front's.
struct StepSet {
    ScratchBuffer keys, words;
    MorphSet view{nullptr, nullptr, 0u};
    void take(StepSet* from) {
        std::swap(keys.p, from->keys.p);
        std::swap(words.p, from->words.p);
        view = from->view;
    }
};

int alloc_set(StepSet* out, uint64_t count, bool with_vals, const char* who) {
    if (int rc = alloc_scratch(&out->keys, size_t(count) * sizeof(uint64_t), who, "a step's keys")) return rc;
    if (with_vals)
        if (int rc = alloc_scratch(&out->words, size_t(count) * sizeof(uint32_t), who, "a step's leaf words")) return rc;
    out->view = MorphSet{out->keys.as<uint64_t>(), with_vals ? out->words.as<uint32_t>() : nullptr, uint32_t(count)};
    return VXRT_OK;
}

// part[blocks] (the scan's total) -> the host.  Waits.
int read_total(const uint64_t* part, uint32_t blocks, hipStream_t s, uint64_t* total) {
    HIP_TRY(hipMemcpyAsync(total, part + blocks, sizeof *total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

// The merge of setops.hip over two sets (b.m may be 0: b.keys is readable all the same) -> *out, exactly sized; an empty result
// leaves out->view.m == 0 and allocates nothing.  Launches: the counting merge, the scan, the emitting merge.  Waits.
int merge_sets(const MorphSet& a, const MorphSet& b, uint32_t op, bool with_vals, hipStream_t s, const char* who, StepSet* out) {
    const std::string w = who;
    const uint64_t items = uint64_t(a.m) + uint64_t(b.m);
    if (items >= (uint64_t(1) << 32)) { set_error(w + ": a step's result has 2^32 voxels or more"); return VXRT_E_INVALID; }
    const uint32_t blocks = setop_blocks(items);
    ScratchBuffer part;
    if (int rc = alloc_scratch(&part, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    SetopArgs m{};
    m.keys_a = a.keys;
    m.words_a = with_vals ? a.words : nullptr;
    m.keys_b = b.keys;
    m.words_b = with_vals && op == kListUnion ? b.words : nullptr;      // DIFFERENCE takes b as a mask
    m.ma = a.m;
    m.mb = b.m;
    m.op = op;
    m.part = part.as<uint64_t>();
    HIP_TRY(launch_setop_merge(m, s));
    HIP_TRY(launch_exclusive_scan(m.part, blocks, s));
    uint64_t count = 0;
    if (int rc = read_total(m.part, blocks, s, &count)) return rc;
    out->view = MorphSet{nullptr, nullptr, 0u};
    if (count == 0) return VXRT_OK;
    if (int rc = alloc_set(out, count, with_vals, who)) return rc;
    m.out_keys = out->keys.as<uint64_t>();
    m.out_words = with_vals ? out->words.as<uint32_t>() : nullptr;
    HIP_TRY(launch_setop_merge(m, s));
    HIP_TRY(hipStreamSynchronize(s));      // part is freed on return
    return VXRT_OK;
}

// One step of ERODE on `in` (in.m > 0) -> *out; an empty result leaves out->view.m == 0.  Launches: the mask, the scan, the write.
int erode_step(const MorphSet& in, uint32_t c, bool tile, bool with_vals, hipStream_t s, const char* who, StepSet* out) {
    const uint32_t blocks = morph_blocks(in.m);
    ScratchBuffer masks, part;
    if (int rc = alloc_scratch(&masks, size_t(in.m) * sizeof(uint32_t), who, "the neighbour masks")) return rc;
    if (int rc = alloc_scratch(&part, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    HIP_TRY(launch_morph_mask(in, c, kMorphErode, tile, masks.as<uint32_t>(), part.as<uint64_t>(), s));
    HIP_TRY(launch_exclusive_scan(part.as<uint64_t>(), blocks, s));
    uint64_t count = 0;
    if (int rc = read_total(part.as<uint64_t>(), blocks, s, &count)) return rc;
    out->view = MorphSet{nullptr, nullptr, 0u};
    if (count == 0) return VXRT_OK;
    if (int rc = alloc_set(out, count, with_vals, who)) return rc;
    HIP_TRY(launch_morph_keep(in, c, masks.as<uint32_t>(), part.as<uint64_t>(), out->keys.as<uint64_t>(),
                              with_vals ? out->words.as<uint32_t>() : nullptr, s));
    HIP_TRY(hipStreamSynchronize(s));      // masks and part are freed on return
    return VXRT_OK;
}

// One step of DILATE on `in` (in.m > 0) -> *out.  Launches: the mask, the scan, the offers, the sort's 21 (7 digits of the 53
// bits), the first offers counted, the scan, the first offers written, and merge_sets' three.
int dilate_step(const MorphSet& in, uint32_t c, bool tile, bool with_vals, hipStream_t s, const char* who, StepSet* out) {
    const std::string w = who;
    const uint32_t blocks = morph_blocks(in.m);
    ScratchBuffer masks, part;
    if (int rc = alloc_scratch(&masks, size_t(in.m) * sizeof(uint32_t), who, "the neighbour masks")) return rc;
    if (int rc = alloc_scratch(&part, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    HIP_TRY(launch_morph_mask(in, c, kMorphDilate, tile, masks.as<uint32_t>(), part.as<uint64_t>(), s));
    HIP_TRY(launch_exclusive_scan(part.as<uint64_t>(), blocks, s));
    uint64_t offers = 0;
    if (int rc = read_total(part.as<uint64_t>(), blocks, s, &offers)) return rc;
    if (offers >= (uint64_t(1) << 32)) { set_error(w + ": a step has 2^32 candidates or more"); return VXRT_E_INVALID; }
    if (offers == 0) { set_error(w + ": internal error: a set without an empty cell beside it"); return VXRT_E_INVALID; }

    // the offers, sorted by (cell, row as the cell sees the source): the first of each cell is its first source
    ListScratch ls;
    ScratchBuffer firsts;
    const uint32_t oblocks = morph_blocks(offers);
    if (int rc = alloc_list_scratch(size_t(offers), with_vals, who, &ls)) return rc;
    if (int rc = alloc_scratch(&firsts, (size_t(oblocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    uint64_t* kp[2] = {ls.keys[0].as<uint64_t>(), ls.keys[1].as<uint64_t>()};
    uint32_t* vp[2] = {ls.vals[0].as<uint32_t>(), ls.vals[1].as<uint32_t>()};
    HIP_TRY(launch_morph_offer(in, c, masks.as<uint32_t>(), part.as<uint64_t>(), kp[0], vp[0], s));
    int at = 0;
    HIP_TRY(radix_sort_pairs(kp, vp, uint32_t(offers), 53u, ls.hist.as<uint32_t>(), ls.totals.as<uint32_t>(), s, &at));
    HIP_TRY(launch_morph_first(kp[at], vp[at], uint32_t(offers), firsts.as<uint64_t>(), nullptr, nullptr, s));
    HIP_TRY(launch_exclusive_scan(firsts.as<uint64_t>(), oblocks, s));
    uint64_t fresh = 0;
    if (int rc = read_total(firsts.as<uint64_t>(), oblocks, s, &fresh)) return rc;
    StepSet cells;
    if (int rc = alloc_set(&cells, fresh, with_vals, who)) return rc;
    HIP_TRY(launch_morph_first(kp[at], vp[at], uint32_t(offers), firsts.as<uint64_t>(), cells.keys.as<uint64_t>(),
                               with_vals ? cells.words.as<uint32_t>() : nullptr, s));
    // the new cells and the set are disjoint: UNION interleaves them
    return merge_sets(in, cells.view, kListUnion, with_vals, s, who, out);
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
    if (with_vals) {
        if ((out_pos != nullptr) != (out_mrgb != nullptr)) { set_error(w + ": out_pos and out_mrgb come both or neither"); return VXRT_E_INVALID; }
    } else if (out_mrgb) {
        set_error(w + ": out_mrgb without mrgb");
        return VXRT_E_INVALID;
    }
    if (n != 0 && !pos) { set_error(w + ": null voxel positions"); return VXRT_E_INVALID; }
    if (n == 0) { *n_out = 0; return VXRT_OK; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_device_array(c, pos, n * 3 * sizeof(int16_t), who, "pos")) return rc;
    if (mrgb)
        if (int rc = check_device_array(c, mrgb, n * 4, who, "mrgb")) return rc;
    if (out_pos)
        if (int rc = check_device_array(c, out_pos, cap * 3 * sizeof(int16_t), who, "out_pos")) return rc;
    if (out_mrgb)
        if (int rc = check_device_array(c, out_mrgb, cap * 4, who, "out_mrgb")) return rc;

    // the list: keys at depth 15 (every int16 position is inside that cube), sorted, one per position, the last entry's bytes.
    // Every input byte is read here, into scratch, before the decode at the end writes the first output byte.  A counting call
    // leaves the leaf words behind: no count depends on them.
    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    const bool vals = with_vals && out_pos != nullptr;
    ListScratch ls;
    ScratchBuffer leaves;
    if (int rc = alloc_list_scratch(n, vals, who, &ls)) return rc;
    ListBounds lb;
    if (int rc = edit_keys_device(reinterpret_cast<const int16_t*>(pos), vals ? reinterpret_cast<const uint8_t*>(mrgb) : nullptr, n, 15u,
                                  ls.keys[0].as<uint64_t>(), vals ? ls.vals[0].as<uint32_t>() : nullptr, s, who, &lb))
        return rc;
    size_t m = 0;
    int cur = 0;
    if (int rc = sort_unique_list(&ls, uint32_t(n), 15u, &leaves, s, who, &m, &cur)) return rc;
    const MorphSet original{ls.keys[cur].as<uint64_t>(), vals ? leaves.as<uint32_t>() : nullptr, uint32_t(m)};      // 0 < m <= n

    // the steps, each on the result of the one before; an eroded set that is empty stays empty
    const bool grow = op == VXRT_MORPH_DILATE || op == VXRT_MORPH_MARGIN;
    const bool tile = c->morph_tile_lookup != 0;      // off in the product: the plain lookup measured faster (vxrt_debug.h has the switch)
    StepSet now;
    now.view = original;
    for (uint32_t step = 0; step < steps && now.view.m != 0u; step++) {
        StepSet next;
        if (int rc = grow ? dilate_step(now.view, connectivity, tile, vals, s, who, &next) : erode_step(now.view, connectivity, tile, vals, s, who, &next)) return rc;
        now.take(&next);      // the set before goes with `next`
    }
    if (op == VXRT_MORPH_SURFACE || op == VXRT_MORPH_MARGIN) {
        ScratchBuffer none;      // an empty set's keys: readable, never used
        if (int rc = alloc_scratch(&none, 0, who, "the keys")) return rc;
        MorphSet mask = grow ? original : now.view;
        if (mask.m == 0u) mask.keys = none.as<uint64_t>();
        StepSet cut;
        if (int rc = merge_sets(grow ? now.view : original, mask, kListDifference, vals, s, who, &cut)) return rc;
        now.take(&cut);
    }

    const uint64_t count = now.view.m;
    *n_out = size_t(count);
    if (!out_pos || count == 0) return VXRT_OK;
    if (count > cap) {
        set_error(w + ": " + std::to_string(count) + " voxels, room for " + std::to_string(cap));
        return VXRT_E_INVALID;
    }
    HIP_TRY(launch_transform_decode(now.view.keys, now.view.words, uint32_t(count), reinterpret_cast<uint8_t*>(out_pos),
                                    reinterpret_cast<uint8_t*>(out_mrgb), s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
} VXRT_CATCH

int vxrt_debug_morph_tile_lookup(vxrt_ctx* c, uint32_t enable) try {
    if (!vxrt::valid_ctx(c)) { vxrt::set_error("null context"); return VXRT_E_INVALID; }
    c->morph_tile_lookup = enable != 0u ? 1 : 0;
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
