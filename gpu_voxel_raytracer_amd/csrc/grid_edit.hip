// grid_edit.hip — device side of vxrt_grid_edit.h: the diff of a dense grid against the scene in one box, emitted as the two
// key-ordered lists of vxrt_edit_voxels (clears, sets) and cut into edit_kernel's segments (edit.h: EditArgs) on the device.  The
// host side is api_grid_edit.hip; DESIGN.md §13.
//
//   outside       SET / REPLACE, a box that leaves the root cube: every cell of the box outside the cube (up to 6 slabs) is read, no
//                 descent; an occupied one raises a flag (a plain store of 1: every writer writes the same word)
//   tile diff     one workgroup per 16-aligned tile of box ∩ root cube (grid_build.hip's tiles): a thread per 16-cell row loads the
//                 row (load_row), finds s(p) by leaf_at's descent for the cells the mode needs, and sums a TileStat (grid.h) of the
//                 tile's clears and sets and the min / max of its set cells per axis -> reduced -> one read-back
//   order         the tile pipeline's order_active_tiles (grid.h): the tiles with an action first, in path order; their packed
//                 (clears, sets) counts scanned in that order
//   emit          one workgroup per active tile: the diff again, staged in LDS in in-tile Morton order, each list ranked by wave
//                 ballots (tile_rank) -> keys (and the sets' words) at the tile's offsets.  Tiles in path order and cells in Morton
//                 order give each list sorted and unique by path key, as api_edit.hip's host sort does
//   cut           per list: the run starts of every level (key >> 3 (L + 1 - l) differs from the previous entry's) counted per chunk
//                 of 4096 entries and level, one flat exclusive scan over [level][chunk] (which is also seg_off), one read-back of
//                 the level counts for both lists, then child_begin and oct written by rank (cut_edit_lists, which
//                 vxrt_edit_voxels_device uses for its one list)
// Every position is a prefix sum; nothing is decided by an atomic, so two calls write the same bytes.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>

#include "block_scan.h"
#include "ctx.h"
#include "grid_edit.h"

namespace vxrt {
namespace {

constexpr uint32_t kThreads = kTileThreads;        // one thread per 16-cell row of a tile (16 x 16 rows)
constexpr uint32_t kWaves = kTileWaves;
constexpr uint32_t kChunk = 4096;                  // list entries per cut chunk (16 per thread)
constexpr uint32_t kOutsideBlocks = 1024;

struct Readback {
    TileStat all;           // count[0]: the clears, count[1]: the sets
    uint32_t outside;       // an occupied cell lies outside the root cube
    uint32_t pad;
};

// The 16 cells p = (px, py, pz0 + k): the grid's words in w[k], the cells to set in bit k of *sets, to clear in bit k of *clears.
__device__ __forceinline__ void row_diff(const GridEdit& e, const uint32_t* pal, int px, int py, int pz0, uint32_t w[16], uint32_t* sets,
                                         uint32_t* clears) {
    load_row(e.g, pal, px, py, pz0, w);
    uint32_t st = 0, cl = 0;
    if (px >= e.clo[0] && px < e.chi[0] && py >= e.clo[1] && py < e.chi[1]) {
        const int half = 1 << e.depth;
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const int pz = pz0 + k;
            const bool occ = (w[k] >> 31) != 0u;
            if (pz < e.clo[2] || pz >= e.chi[2] || (!occ && e.mode != VXRT_GRID_EDIT_REPLACE)) continue;
            const uint32_t s = leaf_at(e.svo, e.leaves, e.depth, uint32_t(px + half), uint32_t(py + half), uint32_t(pz + half));
            if (e.mode == VXRT_GRID_EDIT_CLEAR) cl |= (s != 0u ? 1u : 0u) << k;
            else if (occ) st |= (s != w[k] ? 1u : 0u) << k;
            else cl |= (s != 0u ? 1u : 0u) << k;
        }
    }
    *sets = st;
    *clears = cl;
}

// ---- outside the root cube -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grid_edit_outside_kernel(const GridDesc g, uint64_t i0, uint64_t j0, uint64_t k0, uint64_t ni,
                                                                     uint64_t nj, uint64_t nk, uint32_t* flag) {
    const uint64_t cells = ni * nj * nk;
    for (uint64_t c = uint64_t(blockIdx.x) * kThreads + threadIdx.x; c < cells; c += uint64_t(gridDim.x) * kThreads) {
        const uint64_t k = c % nk, r = c / nk;
        const uint64_t j = r % nj, i = r / nj;
        const size_t at = ((i0 + i) * g.n[1] + (j0 + j)) * g.n[2] + k0 + k;
        const bool occ = g.format == 1u ? static_cast<const uint8_t*>(g.cells)[at] != 0u : (static_cast<const uint32_t*>(g.cells)[at] >> 31) != 0u;
        if (occ) *flag = 1u;
    }
}

// ---- tile diff -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grid_edit_diff_kernel(const GridEdit e, const uint32_t* pal, TileStat* out) {
    __shared__ TileStat lds[kWaves];
    int p0[3];
    tile_origin(e.g, e.small, e.depth, blockIdx.x, p0);
    const int px = p0[0] + int(threadIdx.x >> 4), py = p0[1] + int(threadIdx.x & 15u);
    uint32_t w[16], sets, clears;
    row_diff(e, pal, px, py, p0[2], w, &sets, &clears);
    TileStat v{{uint32_t(__popc(clears)), uint32_t(__popc(sets))}, 0, 0, {INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
    if (sets) {
        v.lo[0] = v.hi[0] = px;
        v.lo[1] = v.hi[1] = py;
        v.lo[2] = p0[2] + __builtin_ctz(sets);
        v.hi[2] = p0[2] + 31 - __builtin_clz(sets);
    }
    block_tile_stat(v, true, lds, out + blockIdx.x);
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------
// Workgroup b: the b-th active tile in path order (order[b]; small: the root cube of a depth < 4 tree, the only tile).  Its cells'
// actions are staged in LDS at their in-tile Morton index and each list ranked by tile_rank; offset[b] packs the tile's first clear
// (low) and first set (high).
__global__ __launch_bounds__(kThreads) void grid_edit_emit_kernel(const GridEdit e, const uint32_t* pal, const uint32_t* order,
                                                                  const uint64_t* offset, uint64_t n_clear, uint64_t n_set, uint64_t* ckeys,
                                                                  uint64_t* skeys, int32_t* swords) {
    __shared__ uint32_t s_word[kTileCells];
    __shared__ uint8_t s_act[kTileCells];          // 1: clear, 2: set
    __shared__ uint32_t s_off[2][kTileRounds * kWaves];
    const uint32_t t = threadIdx.x;
    int p0[3];
    uint64_t code = 0, cat = 0, sat = 0;
    if (e.small) {
        tile_origin(e.g, 1u, e.depth, 0u, p0);
    } else {
        const uint32_t tile = order[blockIdx.x];
        tile_origin(e.g, 0u, e.depth, tile, p0);
        code = tile_code(e.g, tile, e.depth);
        const uint64_t o = offset[blockIdx.x];
        cat = o & 0xffffffffull;
        sat = o >> 32;
    }
    const uint32_t x = t >> 4, y = t & 15u;
    uint32_t w[16], sets, clears;
    row_diff(e, pal, p0[0] + int(x), p0[1] + int(y), p0[2], w, &sets, &clears);
#pragma unroll
    for (uint32_t z = 0; z < 16; z++) {
        const uint32_t mi = morton4(x, y, z);
        s_word[mi] = w[z];
        s_act[mi] = uint8_t((clears >> z & 1u) | (sets >> z & 1u) << 1);
    }
    __syncthreads();
    tile_rank_scan<2>([&](uint32_t j, uint32_t k) { return s_act[j * kThreads + t] == k + 1u; }, s_off);
#pragma unroll
    for (uint32_t j = 0; j < kTileRounds; j++) {
        const uint32_t mi = j * kThreads + t;
        const uint32_t act = s_act[mi];
        const uint64_t key = code << 12 | mi;
        const uint64_t oc = cat + tile_rank(s_off[0], j, act == 1u), os = sat + tile_rank(s_off[1], j, act == 2u);
        // o < n unless the grid changed between the passes (a race of the caller's): then nothing past the lists is written
        if (act == 1u) {
            if (oc < n_clear) ckeys[oc] = key;
        } else if (act == 2u) {
            if (os < n_set) {
                skeys[os] = key;
                swords[os] = int32_t(s_word[mi]);
            }
        }
    }
}

// ---- cut -----------------------------------------------------------------------------------------------------------------------
// The first level at which entry i starts a run: 0 for the first entry; else the levels l with key >> 3 (L + 1 - l) different from
// the previous key's, l >= L + 1 - floor(b / 3) for b the highest differing bit.  0xff past the list.  A list the emit left
// inconsistent (cells rewritten between the two passes) still gives a well-formed cut: edit_kernel then stays inside the scene.
__device__ __forceinline__ void load_cut(const uint64_t* keys, uint32_t m, uint32_t L, uint32_t i0, uint64_t key[16], uint32_t lv[16]) {
    uint64_t prev = i0 > 0u && i0 <= m ? keys[i0 - 1] : 0ull;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        const uint32_t i = i0 + k;
        key[k] = i < m ? keys[i] : 0ull;
        if (i >= m) lv[k] = 0xffu;
        else if (i == 0u) lv[k] = 0u;
        else {   // clamped to [1, L + 1]: one root segment, and every start of a level starts the levels below, whatever the keys
            const uint64_t d = key[k] ^ prev;
            const uint32_t q = d ? uint32_t(63 - __builtin_clzll(d)) / 3u : 0u;
            lv[k] = q >= L ? 1u : L + 1u - q;
        }
        prev = key[k];
    }
}

// part[l * chunks + c] = the run starts of level l (0 .. L + 1) among chunk c's entries
__global__ __launch_bounds__(kThreads) void cut_count_kernel(const uint64_t* keys, uint32_t m, uint32_t L, uint32_t chunks, uint64_t* part) {
    __shared__ uint32_t lds[kWaves];
    uint64_t key[16];
    uint32_t lv[16];
    load_cut(keys, m, L, blockIdx.x * kChunk + threadIdx.x * 16u, key, lv);
    for (uint32_t l = 0; l <= L + 1u; l++) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) n += lv[k] <= l ? 1u : 0u;
        n = wave_sum(n);
        if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = n;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t all = 0;
            for (uint32_t w = 0; w < kWaves; w++) all += lds[w];
            part[size_t(l) * chunks + blockIdx.x] = all;
        }
        __syncthreads();
    }
}

// after the flat exclusive scan of part: seg_off[l] = part[l * chunks], the total at part[(L + 2) * chunks]
__global__ void cut_offsets_kernel(const uint64_t* part, uint32_t L, uint32_t chunks, uint32_t* seg_off) {
    const uint32_t l = threadIdx.x;
    if (l <= L + 2u) seg_off[l] = uint32_t(part[size_t(l) * chunks]);
}

// Entry i, a run start of level l at rank r in that level: segment seg_off[l] + r, whose first child is the segment entry i starts at
// level l + 1; oct = its octant in its parent.  From the entries (level L + 1, segment seg_off[L + 1] + i) up to the root.
__global__ __launch_bounds__(kThreads) void cut_write_kernel(const uint64_t* keys, uint32_t m, uint32_t L, uint32_t chunks, const uint64_t* part,
                                                             uint32_t* child_begin, uint8_t* oct) {
    __shared__ uint32_t lds[kWaves];
    const uint32_t i0 = blockIdx.x * kChunk + threadIdx.x * 16u;
    uint64_t key[16];
    uint32_t lv[16], nxt[16];
    load_cut(keys, m, L, i0, key, lv);
    const uint32_t entries = uint32_t(part[size_t(L + 1u) * chunks]);
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) {
        nxt[k] = entries + i0 + k;
        if (i0 + k < m) oct[entries + i0 + k] = uint8_t(key[k] & 7u);
    }
    for (int l = int(L); l >= 0; l--) {
        uint32_t n = 0;
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) n += lv[k] <= uint32_t(l) ? 1u : 0u;
        uint32_t total;
        uint32_t at = uint32_t(part[size_t(l) * chunks + blockIdx.x]) + block_exclusive<uint32_t, kWaves>(n, lds, &total);
        const uint32_t shift = 3u * (L + 1u - uint32_t(l));
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) {
            if (lv[k] <= uint32_t(l)) {
                child_begin[at] = nxt[k];
                if (l > 0) oct[at] = uint8_t(key[k] >> shift & 7u);
                nxt[k] = at;
                at++;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        oct[0] = 0;
        child_begin[entries] = uint32_t(part[size_t(L + 2u) * chunks]);
    }
}

size_t align16(size_t v) { return (v + 15) & ~size_t(15); }

}  // namespace

int cut_edit_lists(const uint64_t* const* lkeys, const uint32_t* m, int count, uint32_t L, hipStream_t s, const char* who, ScratchBuffer* batch,
                   EditBatch* const* out) {
    // counts per level and chunk, one flat scan per list -> one read-back of every list's seg_off
    constexpr int kMaxLists = 2;
    if (count < 1 || count > kMaxLists) { set_error(std::string(who) + ": internal error: bad list count"); return VXRT_E_INVALID; }
    const uint32_t levels = L + 2u;
    uint32_t chunks[kMaxLists];
    size_t o_part[kMaxLists], part_bytes = 0;
    for (int b = 0; b < count; b++) {
        chunks[b] = (m[b] + kChunk - 1) / kChunk;
        o_part[b] = part_bytes;
        part_bytes += align16((size_t(levels) * chunks[b] + 1) * sizeof(uint64_t));
    }
    ScratchBuffer part, segs;
    if (int rc = alloc_scratch(&part, part_bytes, who, "the level counts")) return rc;
    if (int rc = alloc_scratch(&segs, size_t(count) * 32 * sizeof(uint32_t), who, "the level counts")) return rc;
    HIP_TRY(hipMemsetAsync(segs.get(), 0, size_t(count) * 32 * sizeof(uint32_t), s));
    for (int b = 0; b < count; b++) {
        if (m[b] == 0) continue;
        uint64_t* p = reinterpret_cast<uint64_t*>(part.as<char>() + o_part[b]);
        hipLaunchKernelGGL(cut_count_kernel, dim3(chunks[b]), dim3(kThreads), 0, s, lkeys[b], m[b], L, chunks[b], p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(launch_exclusive_scan(p, levels * chunks[b], s));
        hipLaunchKernelGGL(cut_offsets_kernel, dim3(1), dim3(64), 0, s, p, L, chunks[b], segs.as<uint32_t>() + 32 * b);
        HIP_TRY(hipGetLastError());
    }
    uint32_t seg_off[kMaxLists][32];
    HIP_TRY(hipMemcpyAsync(seg_off, segs.get(), size_t(count) * 32 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    // child_begin | oct of every list, then the edit kernel's scratch (node | flag | out), shared by the launches
    size_t o_cb[kMaxLists], o_oct[kMaxLists], bytes = 0, node_max = 0;
    for (int b = 0; b < count; b++) {
        const size_t node_segs = seg_off[b][L + 1], total = seg_off[b][L + 2];
        o_cb[b] = bytes;
        bytes += align16((node_segs + 1) * 4);
        o_oct[b] = bytes;
        bytes += align16(total);
        node_max = std::max(node_max, node_segs);
    }
    const size_t o_node = bytes, o_flag = o_node + align16(node_max * 4), o_out = o_flag + align16(node_max);
    if (int rc = alloc_scratch(batch, o_out + 8 * 4, who, "the edit batches")) return rc;
    char* base = batch->as<char>();
    for (int b = 0; b < count; b++) {
        if (m[b] == 0) continue;
        const uint64_t* p = reinterpret_cast<const uint64_t*>(part.as<char>() + o_part[b]);
        hipLaunchKernelGGL(cut_write_kernel, dim3(chunks[b]), dim3(kThreads), 0, s, lkeys[b], m[b], L, chunks[b], p,
                           reinterpret_cast<uint32_t*>(base + o_cb[b]), reinterpret_cast<uint8_t*>(base + o_oct[b]));
        HIP_TRY(hipGetLastError());
        EditBatch& eb = *out[b];
        memcpy(eb.seg_off, seg_off[b], sizeof eb.seg_off);
        eb.child_begin = reinterpret_cast<const uint32_t*>(base + o_cb[b]);
        eb.oct = reinterpret_cast<const uint8_t*>(base + o_oct[b]);
        eb.node = reinterpret_cast<uint32_t*>(base + o_node);
        eb.flag = reinterpret_cast<uint8_t*>(base + o_flag);
        eb.out = reinterpret_cast<uint32_t*>(base + o_out);
    }
    HIP_TRY(hipStreamSynchronize(s));   // `part` is freed on return
    return VXRT_OK;
}

int diff_grid_device(const GridEdit& e, const uint32_t* pal, const uint64_t (*outside)[6], uint32_t n_outside, hipStream_t s,
                     GridEditLists* out) {
    const uint64_t ntiles64 = uint64_t(e.g.nt[0]) * e.g.nt[1] * e.g.nt[2];
    if (ntiles64 >= (uint64_t(1) << 31)) { set_error("vxrt_edit_voxel_grid: 2^31 tiles or more"); return VXRT_E_SCENE; }
    const uint32_t ntiles = uint32_t(ntiles64);
    const uint32_t L = e.depth;
    const char* who = "vxrt_edit_voxel_grid";

    // outside the cube, then the tile diff -> one read-back
    ScratchBuffer diff, red;
    if (int rc = alloc_scratch(&diff, size_t(ntiles) * sizeof(TileStat), who, "the tile counts")) return rc;
    if (int rc = alloc_scratch(&red, kTileReduceBlocks * sizeof(TileStat) + sizeof(Readback), who, "the tile counts")) return rc;
    Readback* rb = reinterpret_cast<Readback*>(red.as<TileStat>() + kTileReduceBlocks);
    HIP_TRY(hipMemsetAsync(rb, 0, sizeof(Readback), s));
    for (uint32_t b = 0; b < n_outside; b++) {
        const uint64_t* o = outside[b];
        const uint64_t cells = o[3] * o[4] * o[5];
        const uint64_t blocks = std::min<uint64_t>((cells + kThreads - 1) / kThreads, kOutsideBlocks);
        hipLaunchKernelGGL(grid_edit_outside_kernel, dim3(uint32_t(blocks)), dim3(kThreads), 0, s, e.g, o[0], o[1], o[2], o[3], o[4], o[5],
                           &rb->outside);
        HIP_TRY(hipGetLastError());
    }
    if (ntiles) {
        hipLaunchKernelGGL(grid_edit_diff_kernel, dim3(ntiles), dim3(kThreads), 0, s, e, pal, diff.as<TileStat>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(launch_tile_reduce(diff.as<TileStat>(), ntiles, red.as<TileStat>(), &rb->all, s));
    }
    Readback all;
    HIP_TRY(hipMemcpyAsync(&all, rb, sizeof all, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (all.outside) { set_error("vxrt_edit_voxel_grid: an occupied cell lies outside the scene's root cube"); return VXRT_E_SCENE; }
    const uint64_t n_clear64 = all.all.count[0], n_set64 = all.all.count[1];
    if (n_set64 >= (uint64_t(1) << 32) || n_clear64 >= (uint64_t(1) << 32)) {
        set_error("vxrt_edit_voxel_grid: 2^32 sets or clears or more");
        return VXRT_E_SCENE;
    }
    out->set = n_set64;
    out->cleared = n_clear64;
    if (n_set64 == 0 && n_clear64 == 0) return VXRT_OK;
    const uint32_t n_clear = uint32_t(n_clear64), n_set = uint32_t(n_set64), active = all.all.active;

    // the lists: keys of both, the sets' words
    ScratchBuffer& lists = out->buf[0];
    const size_t o_skeys = align16(size_t(n_clear) * 8), o_words = o_skeys + align16(size_t(n_set) * 8);
    if (int rc = alloc_scratch(&lists, o_words + size_t(n_set) * 4, who, "the lists")) return rc;
    uint64_t* ckeys = lists.as<uint64_t>();
    uint64_t* skeys = reinterpret_cast<uint64_t*>(lists.as<char>() + o_skeys);
    int32_t* swords = reinterpret_cast<int32_t*>(lists.as<char>() + o_words);
    TileOrder tiles;
    if (e.small) {   // the root cube is the one tile
        hipLaunchKernelGGL(grid_edit_emit_kernel, dim3(1), dim3(kThreads), 0, s, e, pal, nullptr, nullptr, uint64_t(n_clear), uint64_t(n_set),
                           ckeys, skeys, swords);
    } else {
        if (int rc = order_active_tiles(e.g, diff.as<TileStat>(), ntiles, active, L, s, who, &tiles)) return rc;
        hipLaunchKernelGGL(grid_edit_emit_kernel, dim3(active), dim3(kThreads), 0, s, e, pal, tiles.order, tiles.offset.as<uint64_t>(),
                           uint64_t(n_clear), uint64_t(n_set), ckeys, skeys, swords);
    }
    HIP_TRY(hipGetLastError());

    // the cut of both lists -> the two batches
    const uint32_t m[2] = {n_clear, n_set};
    const uint64_t* lkeys[2] = {ckeys, skeys};
    EditBatch* eb[2] = {&out->clears, &out->sets};
    if (int rc = cut_edit_lists(lkeys, m, 2, L, s, who, &out->buf[1], eb)) return rc;
    for (int b = 0; b < 2; b++) {
        if (m[b] == 0) continue;
        eb[b]->clear = b == 0;
        eb[b]->words = b == 0 ? nullptr : swords;
        for (int a = 0; a < 3; a++) { eb[b]->lo[a] = all.all.lo[a]; eb[b]->hi[a] = all.all.hi[a]; }
    }
    HIP_TRY(hipStreamSynchronize(s));   // `tiles` is freed on return
    return VXRT_OK;
}

}  // namespace vxrt
