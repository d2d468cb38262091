// api_edit.hip — host side of vxrt_edit.h: in-place scene edits (vxrt_edit_voxels) and the pick query (vxrt_pick).
// The batch is sorted and cut into per-level segments here (the edits are in host memory already, and the cut is key arithmetic
// only); the tree surgery runs on the device (edit.hip: edit_kernel).  DESIGN.md "Scene edits".
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "ctx.h"
#include "edit.h"
#include "query.h"
#include "scene_args.h"

namespace vxrt {
namespace {

// Path key of a voxel: the octants of node levels 0 .. depth, 3 bits each, the root's highest.  Node level l's octant is bit
// (depth - l) of u = coordinate + 2^depth, per axis (x: 4, y: 2, z: 1) — scene_host.cpp: build_octree's "coordinate >= centre".
uint64_t path_key(uint32_t ux, uint32_t uy, uint32_t uz, uint32_t depth) {
    uint64_t k = 0;
    for (int b = int(depth); b >= 0; b--)
        k = k << 3 | uint64_t((ux >> b & 1u) << 2 | (uy >> b & 1u) << 1 | (uz >> b & 1u));
    return k;
}

// stable LSD radix sort of (key, index) by key, 11 bits per pass over the key's `bits`
void sort_by_key(std::vector<uint64_t>& key, std::vector<uint32_t>& idx, uint32_t bits) {
    const size_t n = key.size();
    std::vector<uint64_t> k2(n);
    std::vector<uint32_t> i2(n);
    for (uint32_t shift = 0; shift < bits; shift += 11) {
        std::vector<size_t> count(2049, 0);
        for (size_t i = 0; i < n; i++) count[(key[i] >> shift & 2047u) + 1]++;
        for (size_t b = 1; b < count.size(); b++) count[b] += count[b - 1];
        for (size_t i = 0; i < n; i++) {
            const size_t at = count[key[i] >> shift & 2047u]++;
            k2[at] = key[i];
            i2[at] = idx[i];
        }
        key.swap(k2);
        idx.swap(i2);
    }
}

// a device array of `cap` entries holding the first `used` of `p` (cap > used) and zeros after them (so that the unused entries of
// the 8-entry blocks edits allocate are the same in every context)
template <typename T> hipError_t grow_to(const T* p, size_t used, size_t cap, DeviceBuf<T>* fresh) {
    hipError_t e = fresh->alloc(cap);
    if (e == hipSuccess) e = hipMemcpy(fresh->get(), p, used * sizeof(T), hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipMemset(fresh->get() + used, 0, (cap - used) * sizeof(T));
    return e;
}

// room for `need` entries: geometric growth (x 1.5), and only here
size_t grown_capacity(size_t cap, size_t need) { return std::max(need, cap + cap / 2 + 4096); }

}  // namespace

// the storage for `svo_need` records and `leaf_need` leaf words (edit.h): all or nothing, built in a local and handed over whole
int grow_storage(vxrt_ctx* c, size_t svo_need, size_t leaf_need, GrownStorage* out) {
    GrownStorage g;
    const size_t svo_cap = c->svo_cap ? c->svo_cap : c->svo_count, leaf_cap = c->leaf_cap ? c->leaf_cap : c->leaf_count;
    if (svo_need >= (size_t(1) << 32) || leaf_need >= (size_t(1) << 32)) { set_error("the edited scene would exceed 2^32 records"); return VXRT_E_SCENE; }
    g.svo_cap = svo_need > svo_cap ? grown_capacity(svo_cap, svo_need) : 0;
    g.leaf_cap = leaf_need > leaf_cap ? grown_capacity(leaf_cap, leaf_need) : 0;
    if (g.svo_cap) HIP_TRY(grow_to(c->d_svo.get(), c->svo_count, g.svo_cap, &g.svo));
    if (g.leaf_cap) {
        if (hipError_t e = grow_to(c->d_leaves.get(), c->leaf_count, g.leaf_cap, &g.leaves); e != hipSuccess) return hip_fail(e, "growing the scene's leaf words");
    }
    if (g.svo_cap || g.leaf_cap) HIP_TRY(hipDeviceSynchronize());   // the copies and fills ran on the null stream; the edit runs on c->stream
    *out = std::move(g);
    return VXRT_OK;
}

// the grown storage replaces the old: the same records in larger arrays, so the counts, the touch maps and the DDA grid stay
void commit_storage(vxrt_ctx* c, GrownStorage&& g) {
    if (g.svo) { c->d_svo = std::move(g.svo); c->svo_cap = g.svo_cap; }
    if (g.leaves) { c->d_leaves = std::move(g.leaves); c->leaf_cap = g.leaf_cap; }
}

int reserve_edit_storage(vxrt_ctx* c, size_t nodes, size_t parents) {
    GrownStorage g;
    if (int rc = grow_storage(c, c->svo_count + 8 * nodes, c->leaf_count + 8 * parents, &g)) return rc;
    commit_storage(c, std::move(g));
    return VXRT_OK;
}

int apply_edit_batch(vxrt_ctx* c, const EditBatch& b) {
    const bool clear = b.clear;
    const uint32_t L = c->depth;
    const size_t node_segs = b.seg_off[L + 1];

    // storage: a set may give every touched node of levels 0 .. L-1 a new block of 8 records, every leaf parent 8 leaf words
    const size_t svo_need = clear ? 0 : c->svo_count + 8 * size_t(b.seg_off[L]);
    const size_t leaf_need = clear ? 0 : c->leaf_count + 8 * size_t(b.seg_off[L + 1] - b.seg_off[L]);
    if (svo_need >= (size_t(1) << 32) || leaf_need >= (size_t(1) << 32)) { set_error("the edited scene would exceed 2^32 records"); return VXRT_E_SCENE; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = sync_all(c)) return rc;   // frames enqueued before the edit see the old scene
    GrownStorage grown;
    if (int rc = grow_storage(c, svo_need, leaf_need, &grown)) return rc;
    // host batches: one scratch of  the arrays | node scratch | flag scratch | out
    const size_t o_node = (b.host_bytes + 3) & ~size_t(3), o_flag = o_node + node_segs * 4;
    const size_t o_out = (o_flag + node_segs + 15) & ~size_t(15), bytes = o_out + 8 * 4;
    ScratchBuffer scratch;
    if (b.host) {
        if (hipError_t e = scratch.alloc(bytes); e != hipSuccess) return hip_fail(e, "edit batch");
    }
    // from here on the edit happens
    commit_storage(c, std::move(grown));
    if (!c->edited) { c->edited = true; c->svo_built = c->svo_count; c->leaf_built = c->leaf_count; }
    EditArgs a{};
    memcpy(a.seg_off, b.seg_off, sizeof a.seg_off);
    if (b.host) {
        char* s = scratch.as<char>();
        HIP_TRY(hipMemcpy(s, b.host, b.host_bytes, hipMemcpyHostToDevice));
        a.child_begin = reinterpret_cast<const uint32_t*>(s);
        a.words = reinterpret_cast<const int32_t*>(s + b.host_words);
        a.oct = reinterpret_cast<const uint8_t*>(s + b.host_oct);
        a.node = reinterpret_cast<uint32_t*>(s + o_node);
        a.flag = reinterpret_cast<uint8_t*>(s + o_flag);
        a.out = reinterpret_cast<uint32_t*>(s + o_out);
    } else {
        a.child_begin = b.child_begin;
        a.words = b.words;
        a.oct = b.oct;
        a.node = b.node;
        a.flag = b.flag;
        a.out = b.out;
    }
    a.svo = c->d_svo;
    a.leaves = c->d_leaves;
    a.depth = L;
    a.svo_end = uint32_t(c->svo_count);
    a.leaf_end = uint32_t(c->leaf_count);
    a.svo_built = uint32_t(c->svo_built);
    a.leaf_built = uint32_t(c->leaf_built);
    a.clear = clear ? 1 : 0;
    const bool was_empty = (c->root_rec.masks & 0xffffu) == 0u;
    HIP_TRY(launch_edit(a, c->stream));
    uint32_t out[8];
    HIP_TRY(hipMemcpyAsync(out, a.out, sizeof out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->svo_count = out[0];
    c->leaf_count = out[1];
    c->live_nodes = clear ? c->live_nodes - out[2] : c->live_nodes + out[2];
    c->root_rec = SvoRecord{out[3], out[4]};
    drop_touch_maps(c);   // sized for the records before the edit; the DDA prototype's grid is of the old scene

    // the sky cull's box grows to hold every set voxel's cell of level min(depth, 7); a clear never shrinks it (the cull is exact
    // for any box that holds the scene).  A scene without a box keeps none (its top levels were too large to read back), unless it
    // was empty: then the set voxels are all of it.  A cell's bounds are monotone in its position, so the set voxels' least and
    // greatest positions per axis give the box that growing it voxel by voxel gives.
    if (!clear && (c->box_valid || was_empty)) {
        const uint32_t Lc = L < 7u ? L : 7u;
        const float cell = ldexpf(c->root_size, -int(Lc));
        const int32_t half = int32_t(1) << L;
        for (int ax = 0; ax < 3; ax++) {
            const float root_min = c->root_center[ax] - 0.5f * c->root_size;
            const uint32_t clo = uint32_t(b.lo[ax] + half) >> (L + 1 - Lc), chi = uint32_t(b.hi[ax] + half) >> (L + 1 - Lc);
            const float lo = root_min + float(clo) * cell, hi = root_min + float(chi + 1u) * cell;
            c->box_min[ax] = c->box_valid ? std::min(c->box_min[ax], lo) : lo;
            c->box_max[ax] = c->box_valid ? std::max(c->box_max[ax], hi) : hi;
        }
        c->box_valid = true;
    }
    return VXRT_OK;
}

}  // namespace vxrt

extern "C" {

int vxrt_edit_voxels(vxrt_ctx* c, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n) try {
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (n != 0 && !pos) { set_error("null voxel positions"); return VXRT_E_INVALID; }
    if (int rc = require_scene(c)) return rc;
    if (n == 0) return VXRT_OK;
    if (int rc = require_editable_scene(c)) return rc;
    const bool clear = mrgb == nullptr;
    const uint32_t L = c->depth;
    const int32_t half = int32_t(1) << L;

    // keys, refused as a whole when one position lies outside the root cube [-2^d, 2^d)^3
    std::vector<uint64_t> key(n);
    std::vector<uint32_t> idx(n);
    for (size_t i = 0; i < n; i++) {
        uint32_t u[3];
        for (int a = 0; a < 3; a++) {
            const int32_t v = int32_t(pos[i][a]) + half;
            if (v < 0 || v >= 2 * half) {
                set_error("voxel (" + std::to_string(pos[i][0]) + ", " + std::to_string(pos[i][1]) + ", " + std::to_string(pos[i][2]) +
                          ") lies outside the scene's root cube [-" + std::to_string(half) + ", " + std::to_string(half) + ")^3");
                return VXRT_E_SCENE;
            }
            u[a] = uint32_t(v);
        }
        key[i] = path_key(u[0], u[1], u[2], L);
        idx[i] = uint32_t(i);
    }
    sort_by_key(key, idx, 3 * (L + 1));
    // one entry per position: the last of each run (the sort is stable, so that is the batch's last entry for the position)
    size_t m = 0;
    for (size_t i = 0; i < n; i++) {
        if (i + 1 < n && key[i + 1] == key[i]) continue;
        key[m] = key[i];
        idx[m] = idx[i];
        m++;
    }
    key.resize(m);
    idx.resize(m);

    // segments per level (edit.h: EditArgs): level l's are the runs of equal key >> 3 (L + 1 - l); first[] = a run's first entry
    const uint32_t levels = L + 2;   // node levels 0 .. L, then the entries
    std::vector<std::vector<uint32_t>> first(levels);
    for (uint32_t l = 0; l < levels; l++) {
        const uint32_t shift = 3 * (L + 1 - l);
        for (size_t i = 0; i < m; i++)
            if (i == 0 || key[i] >> shift != key[i - 1] >> shift) first[l].push_back(uint32_t(i));
    }
    EditArgs a{};
    a.seg_off[0] = 0;
    for (uint32_t l = 0; l < levels; l++) a.seg_off[l + 1] = a.seg_off[l] + uint32_t(first[l].size());
    const size_t node_segs = a.seg_off[L + 1], total = a.seg_off[L + 2];
    std::vector<uint32_t> child_begin(node_segs + 1);
    std::vector<uint8_t> oct(total, 0);
    for (uint32_t l = 0; l < levels; l++) {
        const uint32_t shift = 3 * (L + 1 - l);
        for (size_t j = 0; j < first[l].size(); j++) {
            if (l > 0) oct[a.seg_off[l] + j] = uint8_t(key[first[l][j]] >> shift & 7u);
            if (l + 1 < levels) {   // its first child starts at the same entry (the next level's runs refine this level's)
                const auto& next = first[l + 1];
                child_begin[a.seg_off[l] + j] = a.seg_off[l + 1] + uint32_t(std::lower_bound(next.begin(), next.end(), first[l][j]) - next.begin());
            }
        }
    }
    child_begin[node_segs] = uint32_t(total);

    EditBatch b;
    memcpy(b.seg_off, a.seg_off, sizeof b.seg_off);
    b.clear = clear;
    // the batch (one upload): child_begin | words | oct
    std::vector<int32_t> words(clear ? 0 : m);
    for (size_t i = 0; i < words.size(); i++) {
        const uint8_t* v = mrgb[idx[i]];
        words[i] = int32_t(0x80000000u | uint32_t(v[0] & 0x7f) << 24 | uint32_t(v[1]) << 16 | uint32_t(v[2]) << 8 | v[3]);
    }
    b.host_words = (node_segs + 1) * 4;
    b.host_oct = b.host_words + words.size() * 4;
    b.host_bytes = b.host_oct + total;
    std::vector<uint8_t> host(b.host_bytes, 0);
    memcpy(host.data(), child_begin.data(), child_begin.size() * 4);
    memcpy(host.data() + b.host_words, words.data(), words.size() * 4);
    memcpy(host.data() + b.host_oct, oct.data(), total);
    b.host = host.data();
    // the set voxels' bounds (the sky cull's box)
    for (int ax = 0; ax < 3; ax++) { b.lo[ax] = INT32_MAX; b.hi[ax] = INT32_MIN; }
    for (size_t i = 0; i < m; i++)
        for (int ax = 0; ax < 3; ax++) {
            b.lo[ax] = std::min(b.lo[ax], int32_t(pos[idx[i]][ax]));
            b.hi[ax] = std::max(b.hi[ax], int32_t(pos[idx[i]][ax]));
        }
    return apply_edit_batch(c, b);
} VXRT_CATCH

int vxrt_pick(vxrt_ctx* c, const float (*origins)[3], const float (*dirs)[3], size_t n, vxrt_pick_hit* out) try {
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (n != 0 && (!origins || !dirs || !out)) { set_error("null argument"); return VXRT_E_INVALID; }
    if (!c->has_scene) { set_error("no scene set"); return VXRT_E_NOSCENE; }
    if (n == 0) return VXRT_OK;
    if (n >= (size_t(1) << 31)) { set_error("too many rays"); return VXRT_E_INVALID; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = vxrt_sync(c)) return rc;
    ScratchBuffer b_o, b_d, b_out;
    HIP_TRY(b_o.alloc(n * 12));
    HIP_TRY(b_d.alloc(n * 12));
    HIP_TRY(b_out.alloc(n * sizeof(vxrt_pick_hit)));
    HIP_TRY(hipMemcpy(b_o.get(), origins, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(b_d.get(), dirs, n * 12, hipMemcpyHostToDevice));
    HIP_TRY(launch_query_pick(pick_args(c), b_o.as<float>(), b_d.as<float>(), nullptr, b_out.as<vxrt_pick_hit>(), unsigned(n), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, b_out.get(), n * sizeof(vxrt_pick_hit), hipMemcpyDeviceToHost));
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
