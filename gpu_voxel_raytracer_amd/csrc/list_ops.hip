// list_ops.hip — list_ops.h's host pipeline: no kernel of its own.
#include "list_ops.h"

#include <algorithm>
#include <string>

#include "run_heads.h"
#include "scene_args.h"
#include "transform.h"

namespace vxrt {

int scan_total(uint64_t* part, uint32_t blocks, hipStream_t s, uint64_t* total) {
    HIP_TRY(launch_exclusive_scan(part, blocks, s));
    HIP_TRY(hipMemcpyAsync(total, part + blocks, sizeof *total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

int alloc_part(ScratchBuffer* part, uint64_t count, const char* who) {
    return alloc_scratch(part, (size_t(morph_blocks(count)) + 1) * sizeof(uint64_t), who, "the block counts");
}

int run_heads_count(const uint64_t* keys, uint32_t n, uint32_t shift, hipStream_t s, const char* who, RunHeads* rh) {
    rh->keys = keys;
    rh->n = n;
    rh->shift = shift;
    if (int rc = alloc_part(&rh->part, n, who)) return rc;
    HIP_TRY(launch_run_heads(keys, nullptr, n, shift, rh->part.as<uint64_t>(), nullptr, nullptr, s));
    return scan_total(rh->part.as<uint64_t>(), morph_blocks(n), s, &rh->count);
}

int run_heads_emit(const RunHeads& rh, const uint32_t* words, uint64_t* out_keys, uint32_t* out_words, hipStream_t s) {
    HIP_TRY(launch_run_heads(rh.keys, words, rh.n, rh.shift, rh.part.as<uint64_t>(), out_keys, out_words, s));
    return VXRT_OK;
}

int run_heads(const uint64_t* keys, const uint32_t* words, uint32_t n, uint32_t shift, bool with_words, hipStream_t s, const char* who,
              const char* whose, RunHeads* rh, OwnedSet* out) {
    if (int rc = run_heads_count(keys, n, shift, s, who, rh)) return rc;
    if (int rc = alloc_set(out, rh->count, with_words, who, whose)) return rc;
    return run_heads_emit(*rh, words, out->keys.as<uint64_t>(), out->words.as<uint32_t>(), s);
}

uint32_t tile_sort_bits(const uint32_t first[3], const uint32_t last[3]) {
    uint32_t bits = 0;
    for (int ax = 0; ax < 3; ax++) {
        uint32_t length = 0;      // the bit length of first ^ last
        while ((first[ax] ^ last[ax]) >> length) length++;
        bits = std::max(bits, 3u * length);
    }
    return bits;
}

int key_list(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, bool with_vals, hipStream_t s, const char* who, KeyedList* out,
             ListBounds* bounds) {
    if (n == 0) {
        if (int rc = alloc_scratch(&out->ls.key[0], 0, who, "the keys")) return rc;
        if (with_vals)
            if (int rc = alloc_scratch(&out->leaves, 0, who, "the leaf words")) return rc;
        out->view = MorphSet{out->ls.keys(), with_vals ? out->leaves.as<uint32_t>() : nullptr, 0u};
        return VXRT_OK;
    }
    if (int rc = alloc_list_scratch(n, with_vals, who, &out->ls)) return rc;
    // keys at depth 15: every int16 position is inside that cube
    ListBounds lb;
    if (int rc = edit_keys_device(reinterpret_cast<const int16_t*>(pos), with_vals ? reinterpret_cast<const uint8_t*>(mrgb) : nullptr, n, 15u,
                                  out->ls.keys(), out->ls.vals(), s, who,
                                  bounds ? bounds : &lb))
        return rc;
    size_t m = 0;
    if (int rc = sort_unique_list(&out->ls, uint32_t(n), 15u, &out->leaves, s, who, &m)) return rc;
    out->view = MorphSet{out->ls.keys(), with_vals ? out->leaves.as<uint32_t>() : nullptr, uint32_t(m)};      // 0 < m <= n
    return VXRT_OK;
}

int alloc_set(OwnedSet* out, uint64_t count, bool with_vals, const char* who, const char* whose) {
    if (int rc = alloc_scratch(&out->keys, size_t(count) * sizeof(uint64_t), who, (std::string(whose) + " keys").c_str())) return rc;
    if (with_vals)
        if (int rc = alloc_scratch(&out->words, size_t(count) * sizeof(uint32_t), who, (std::string(whose) + " leaf words").c_str())) return rc;
    out->view = MorphSet{out->keys.as<uint64_t>(), with_vals ? out->words.as<uint32_t>() : nullptr, uint32_t(count)};
    return VXRT_OK;
}

int merge_count(const MorphSet& a, const MorphSet& b, uint32_t op, hipStream_t s, const char* who, SetMerge* mg) {
    const uint32_t blocks = setop_blocks(uint64_t(a.m) + uint64_t(b.m));
    if (int rc = alloc_scratch(&mg->part, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    mg->args = SetopArgs{a.keys, a.words, b.keys, b.words, a.m, b.m, op, mg->part.as<uint64_t>(), nullptr, nullptr};
    HIP_TRY(launch_setop_merge(mg->args, s));
    return scan_total(mg->args.part, blocks, s, &mg->count);
}

int merge_emit(SetMerge* mg, hipStream_t s, const char* who, const char* whose, OwnedSet* out) {
    if (int rc = alloc_set(out, mg->count, mg->args.words_a != nullptr, who, whose)) return rc;
    mg->args.out_keys = out->keys.as<uint64_t>();
    mg->args.out_words = out->words.as<uint32_t>();      // null without words
    HIP_TRY(launch_setop_merge(mg->args, s));
    return VXRT_OK;
}

int check_output_pair(bool with_vals, const void* out_pos, const void* out_mrgb, const char* who, const char* input) {
    if (with_vals ? (out_pos != nullptr) != (out_mrgb != nullptr) : out_mrgb != nullptr) {
        set_error(std::string(who) + (with_vals ? ": out_pos and out_mrgb come both or neither" : std::string(": out_mrgb without ") + input));
        return VXRT_E_INVALID;
    }
    return VXRT_OK;
}

int check_input_list(const vxrt_ctx* c, const void* pos, const void* mrgb, size_t n, const char* who, const char* pos_name, const char* mrgb_name) {
    if (n == 0) return VXRT_OK;
    if (int rc = check_device_array(c, pos, n * 3 * sizeof(int16_t), who, pos_name)) return rc;
    return mrgb ? check_device_array(c, mrgb, n * 4, who, mrgb_name) : VXRT_OK;
}

int check_output_arrays(const vxrt_ctx* c, const void* out_pos, const void* out_mrgb, size_t cap, const char* who) {
    if (out_pos)
        if (int rc = check_device_array(c, out_pos, cap * 3 * sizeof(int16_t), who, "out_pos")) return rc;
    if (out_mrgb)
        if (int rc = check_device_array(c, out_mrgb, cap * 4, who, "out_mrgb")) return rc;
    return VXRT_OK;
}

int list_room(uint64_t count, const void* out_pos, size_t cap, const char* who, size_t* n_out) {
    *n_out = size_t(count);
    if (out_pos && count > cap) {
        set_error(std::string(who) + ": " + std::to_string(count) + " voxels, room for " + std::to_string(cap));
        return VXRT_E_INVALID;
    }
    return VXRT_OK;
}

int decode_list(const uint64_t* keys, const uint32_t* words, uint64_t count, int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], hipStream_t s) {
    HIP_TRY(launch_transform_decode(keys, words, uint32_t(count), reinterpret_cast<uint8_t*>(out_pos), reinterpret_cast<uint8_t*>(out_mrgb), s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

}  // namespace vxrt
