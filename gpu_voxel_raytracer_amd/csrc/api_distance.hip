// api_distance.hip — host side of vxrt_distance.h: the exact squared Euclidean distance transform of a voxel list in device memory
// and the ball dilation and erosion a threshold on it gives.  The list is keyed, sorted and deduplicated by list_ops.h's key_list;
// distance.hip's run heads give the tiles of the list; for FIELD and DILATE their 3 x 3 x 3 windows are sorted by a KeySort
// (device_build.h) over the key bits in which they can differ (tile_sort_bits), and the heads of that are the candidate tiles;
// distance.hip then counts per candidate tile, scan_total turns the counts into offsets, and the same kernel writes the caller's
// arrays at them: no keys, no sort and no decode of the result (api_shape.hip's scheme).  The output checks are list_ops.h's.
// Nothing but counts crosses to the host.  The heads are distance.hip's own kernel, one entry a thread, and not run_heads.hip's:
// with that one FIELD and DILATE measured slower than before.  DESIGN.md §30.
#include <algorithm>
#include <string>

#include "distance.h"
#include "list_ops.h"
#include "scene_args.h"
#include "../../include/vxrt_distance.h"

extern "C" {

int vxrt_distance_voxels_device(vxrt_ctx* c, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, uint32_t mode, uint32_t max_d2,
                                int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4], uint16_t* out_d2, size_t cap, size_t* n_out) try {
    using namespace vxrt;
    const char* who = "vxrt_distance_voxels_device";
    const std::string w = who;
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error(w + ": 2^32 voxels or more"); return VXRT_E_INVALID; }
    if (!n_out) { set_error(w + ": null n_out"); return VXRT_E_INVALID; }
    if (mode > uint32_t(VXRT_DISTANCE_DILATE)) { set_error(w + ": mode is no vxrt_distance_mode"); return VXRT_E_INVALID; }
    if (max_d2 < 1u || max_d2 > kDistanceMaxD2) { set_error(w + ": max_d2 must lie in 1 .. 256"); return VXRT_E_INVALID; }
    const bool with_vals = mrgb != nullptr;
    if (int rc = check_output_pair(with_vals, out_pos, out_mrgb, who, "mrgb")) return rc;
    if (out_d2 && !out_pos) { set_error(w + ": out_d2 without out_pos"); return VXRT_E_INVALID; }
    if (n != 0 && !pos) { set_error(w + ": null voxel positions"); return VXRT_E_INVALID; }
    if (n == 0) { *n_out = 0; return VXRT_OK; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_input_list(c, pos, mrgb, n, who, "pos", "mrgb")) return rc;
    if (int rc = check_output_arrays(c, out_pos, out_mrgb, cap, who)) return rc;
    if (out_d2)
        if (int rc = check_device_array(c, out_d2, cap * sizeof(uint16_t), who, "out_d2")) return rc;

    // the list: sorted, one key per position, the last entry's bytes.  Every input byte is read here, into scratch, before the
    // emitting launch at the end writes the first output byte.  A counting call leaves the leaf words behind: no count depends on them.
    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    const bool vals = with_vals && out_pos != nullptr;
    KeyedList list;
    ListBounds box;
    if (int rc = key_list(pos, mrgb, n, vals, s, who, &list, &box)) return rc;
    const uint32_t m = list.view.m;      // 0 < m <= n

    // the tiles of S: the heads of the runs of keys that agree above their low 12 bits
    const bool grow = mode == VXRT_DISTANCE_FIELD || mode == VXRT_DISTANCE_DILATE;
    ScratchBuffer heads;
    if (int rc = alloc_scratch(&heads, (size_t(distance_head_blocks(m)) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
    HIP_TRY(launch_distance_heads(list.view.keys, m, 12u, grow, heads.as<uint64_t>(), nullptr, s));
    uint64_t own = 0;
    if (int rc = scan_total(heads.as<uint64_t>(), distance_head_blocks(m), s, &own)) return rc;
    const uint64_t spread = grow ? own * kDistanceWindowTiles : own;
    if (spread >= (uint64_t(1) << 32)) { set_error(w + ": 2^32 candidate tiles or more"); return VXRT_E_INVALID; }

    // two buffers of spread + 1 words: the sort's ping-pong; then the candidate tiles and their counts
    KeySort tiles;
    if (int rc = tiles.alloc_keys(size_t(spread) + 1, who, "the tiles' keys and counts")) return rc;
    HIP_TRY(launch_distance_heads(list.view.keys, m, 12u, grow, heads.as<uint64_t>(), tiles.keys(), s));

    DistanceArgs a{};
    ScratchBuffer firsts;      // outlives the launches that use it: every path below waits before it returns
    if (!grow) {
        a.ntiles = uint32_t(own);
    } else {
        // the windows' tiles differ in the bits in which the list's box, one tile wider, does
        uint32_t first[3], last[3];
        for (int ax = 0; ax < 3; ax++) {
            const uint32_t lo = uint32_t(box.lo[ax] + 32768) >> 4, hi = uint32_t(box.hi[ax] + 32768) >> 4;
            first[ax] = lo != 0u ? lo - 1u : 0u;
            last[ax] = std::min(hi + 1u, 4095u);
        }
        const uint32_t blocks = distance_head_blocks(spread);
        if (int rc = tiles.alloc_counts(size_t(spread), who)) return rc;
        if (int rc = alloc_scratch(&firsts, (size_t(blocks) + 1) * sizeof(uint64_t), who, "the block counts")) return rc;
        HIP_TRY(tiles.sort(uint32_t(spread), tile_sort_bits(first, last), s));
        // the candidate tiles: the distinct ones, written over the sort's free side
        HIP_TRY(launch_distance_heads(tiles.keys(), uint32_t(spread), 0u, false, firsts.as<uint64_t>(), nullptr, s));
        uint64_t unique = 0;
        if (int rc = scan_total(firsts.as<uint64_t>(), blocks, s, &unique)) return rc;
        HIP_TRY(launch_distance_heads(tiles.keys(), uint32_t(spread), 0u, false, firsts.as<uint64_t>(), tiles.spare_keys(), s));
        tiles.flip();      // the sorted side is read no more once the heads are written, in stream order
        a.ntiles = uint32_t(unique);
    }
    a.tiles = tiles.keys();
    a.part = tiles.spare_keys();
    if (a.ntiles >= (uint32_t(1) << 31)) { set_error(w + ": 2^31 candidate tiles or more"); return VXRT_E_INVALID; }

    a.keys = list.view.keys;
    a.words = nullptr;
    a.m = m;
    a.steps = distance_steps(m);
    a.mode = mode;
    a.max_d2 = max_d2;
    a.radius = distance_radius(max_d2);
    HIP_TRY(launch_distance(a, s));
    uint64_t count = 0;
    if (int rc = scan_total(a.part, a.ntiles, s, &count)) return rc;
    if (count >= (uint64_t(1) << 32)) { set_error(w + ": a result of 2^32 voxels or more"); return VXRT_E_INVALID; }
    if (int rc = list_room(count, out_pos, cap, who, n_out)) return rc;
    if (!out_pos || count == 0) return VXRT_OK;

    a.words = list.view.words;      // nullptr: positions only
    a.out_pos = reinterpret_cast<uint8_t*>(out_pos);
    a.out_mrgb = reinterpret_cast<uint8_t*>(out_mrgb);
    a.out_d2 = reinterpret_cast<uint8_t*>(out_d2);
    HIP_TRY(launch_distance(a, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
