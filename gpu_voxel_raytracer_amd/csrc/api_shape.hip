// api_shape.hip — host side of vxrt_shape.h: a box, ball, cylinder or capsule rasterised into a voxel list in device memory under
// a fixed-point affine pull.  The tiles that meet the box are keyed by shape.hip and sorted by a KeySort (device_build.h) over the
// key bits in which they differ (list_ops.h's tile_sort_bits); shape.hip then counts per tile, scan_total turns the counts into offsets,
// and the same kernel writes the caller's arrays at them: no keys, no sort and no decode of the result.  The output checks are
// list_ops.h's.  Nothing but the count crosses to the host.  DESIGN.md §29.
#include <algorithm>
#include <string>

#include "list_ops.h"
#include "scene_args.h"
#include "shape.h"
#include "shape_rule.h"
#include "../../include/vxrt_shape.h"

extern "C" {

int vxrt_shape_voxels_device(vxrt_ctx* c, const vxrt_shape* shape, const vxrt_affine* pull, const int32_t box_min[3], const int32_t box_max[3],
                             const uint8_t mrgb[4], int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], size_t cap, size_t* n_out) try {
    using namespace vxrt;
    const char* who = "vxrt_shape_voxels_device";
    const std::string w = who;
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (!shape || !pull || !n_out || !box_min || !box_max) { set_error(w + ": null argument"); return VXRT_E_INVALID; }
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
    const uint32_t limit = uint32_t(1) << 29;
    if (shape->kind > VXRT_SHAPE_CAPSULE) { set_error(w + ": shape->kind is not a vxrt_shape_kind"); return VXRT_E_INVALID; }
    if (shape->r > limit || shape->h[0] > limit || shape->h[1] > limit || shape->h[2] > limit) {
        set_error(w + ": shape->r or an entry of shape->h beyond 2^29 (8192 cells in Q16)");
        return VXRT_E_INVALID;
    }
    const bool has_r = shape->kind != VXRT_SHAPE_BOX, has_hxy = shape->kind == VXRT_SHAPE_BOX,
               has_hz = shape->kind != VXRT_SHAPE_BALL;
    if ((!has_r && shape->r != 0) || (!has_hxy && (shape->h[0] != 0 || shape->h[1] != 0)) || (!has_hz && shape->h[2] != 0)) {
        set_error(w + ": a field of the shape that its kind does not use must be 0");
        return VXRT_E_INVALID;
    }
    if (shape->reserved[0] != 0 || shape->reserved[1] != 0 || shape->reserved[2] != 0) {
        set_error(w + ": shape->reserved must be 0");
        return VXRT_E_INVALID;
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
    if (int rc = check_output_pair(mrgb != nullptr, out_pos, out_mrgb, who, "mrgb")) return rc;
    if (empty_box) { *n_out = 0; return VXRT_OK; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_output_arrays(c, out_pos, out_mrgb, cap, who)) return rc;

    ShapeArgs a{};
    uint64_t tiles = 1;
    uint32_t first[3], last[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) a.m[i][j] = pull->m[i][j];
        a.t[i] = pull->t[i];
        a.h2[i] = 2 * int64_t(shape->h[i]);
        a.lo[i] = box_min[i];
        a.hi[i] = box_max[i];
        first[i] = uint32_t(box_min[i] + 32768) >> 4;
        last[i] = uint32_t(box_max[i] - 1 + 32768) >> 4;
        a.tlo[i] = first[i];
        a.text[i] = last[i] - first[i] + 1u;
        tiles *= a.text[i];                                       // each at most 4096, and a box below 2^32 cells has about 2^24 at the most
    }
    const uint32_t sort_bits = tile_sort_bits(first, last);
    if (tiles >= (uint64_t(1) << 31)) { set_error(w + ": too many tiles"); return VXRT_E_INVALID; }
    a.kind = shape->kind;
    a.r2 = 2 * int64_t(shape->r);
    a.reach[0] = a.reach[1] = shape->kind == VXRT_SHAPE_BOX ? a.h2[0] : a.r2;
    if (shape->kind == VXRT_SHAPE_BOX) a.reach[1] = a.h2[1];
    a.reach[2] = shape->kind == VXRT_SHAPE_BALL ? a.r2 : shape->kind == VXRT_SHAPE_CAPSULE ? a.h2[2] + a.r2 : a.h2[2];
    a.tiles = uint32_t(tiles);
    if (mrgb) a.word = (uint32_t(mrgb[0]) & 0x7fu) << 24 | uint32_t(mrgb[1]) << 16 | uint32_t(mrgb[2]) << 8 | uint32_t(mrgb[3]);

#ifdef VXRT_SHAPE_SORTED
    // the A/B route (shape.h): count per block of cells, emit keys in thread order, sort them, decode
    {
        hipStream_t s = c->stream;
        a.cells = uint32_t(cells);
        for (int i = 0; i < 3; i++) a.ext[i] = uint32_t(box_max[i] - box_min[i]);
        const uint32_t blocks = shape_blocks(cells);
        ScratchBuffer part;
        if (int rc = alloc_scratch(&part, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;      // shape_blocks' span
        a.part = part.as<uint64_t>();
        HIP_TRY(launch_shape_linear(a, s));
        uint64_t count = 0;
        if (int rc = scan_total(a.part, blocks, s, &count)) return rc;
        if (int rc = list_room(count, out_pos, cap, who, n_out)) return rc;
        if (!out_pos || count == 0) return VXRT_OK;
        KeySort out;
        if (int rc = out.alloc(size_t(count), false, who)) return rc;
        a.out_keys = out.keys();
        HIP_TRY(launch_shape_linear(a, s));
        HIP_TRY(out.sort(uint32_t(count), 12u + sort_bits, s));
        HIP_TRY(launch_shape_decode(out.keys(), uint32_t(count), a.word, reinterpret_cast<uint8_t*>(out_pos), reinterpret_cast<uint8_t*>(out_mrgb), s));
        HIP_TRY(hipStreamSynchronize(s));
        return VXRT_OK;
    }
#else
    // the scratch, all of it: two buffers of tiles + 1 words (the sort's ping-pong; then the sorted keys and the counts) and the
    // sort's digit counts
    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    KeySort keys;
    if (int rc = keys.alloc_keys(size_t(a.tiles) + 1, who, "the tiles' keys and counts")) return rc;
    if (int rc = keys.alloc_counts(a.tiles, who)) return rc;
    a.keys = keys.keys();
    HIP_TRY(launch_shape_tiles(a, s));
    HIP_TRY(keys.sort(a.tiles, sort_bits, s));
    a.keys = keys.keys();
    a.part = keys.spare_keys();
    HIP_TRY(launch_shape(a, s));
    uint64_t count = 0;
    if (int rc = scan_total(a.part, a.tiles, s, &count)) return rc;
    if (int rc = list_room(count, out_pos, cap, who, n_out)) return rc;
    if (!out_pos || count == 0) return VXRT_OK;

    a.out_pos = reinterpret_cast<uint8_t*>(out_pos);
    a.out_mrgb = reinterpret_cast<uint8_t*>(out_mrgb);
    HIP_TRY(launch_shape(a, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
#endif
} VXRT_CATCH

}  // extern "C"
