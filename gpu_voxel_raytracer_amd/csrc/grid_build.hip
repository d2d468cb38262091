// grid_build.hip — device side of vxrt_grid.h: a scene built from a dense grid of cells (vxrt_set_voxel_grid), and a box of the scene
// written back as a dense grid of leaf words (vxrt_get_voxel_grid).  The host side is api_grid.hip; DESIGN.md §12.
//
// Import.  With d the depth and u = p + 2^d, a 16-aligned tile of p is a 16-aligned tile of u whenever d >= 4 (2^d is a multiple of
// 16), and a voxel's path key is (the Morton code of its u-tile) << 12 | (the Morton code of its cell in the tile).  So the occupied
// cells, taken tile by tile in ascending tile code and in Morton order inside each tile, are already the sorted, unique key list the
// list builder makes with its radix sort and dedupe (device_build.hip); only the tiles need sorting, about one per 4096 cells.
//   tile stats    one workgroup per 16-aligned tile of the grid's box: a TileStat (grid.h) of its occupied count and their min / max
//                 per axis (build_octree's depth rule takes the min and max over the axes) -> reduced -> the depth, the total
//   order         the tile pipeline's order_active_tiles (grid.h, below): the occupied tiles keyed by the Morton code of their
//                 u-tile (d >= 4), the empty ones past every code -> radix_sort_pairs (3(d - 3) + 1 bits) -> the occupied tiles in
//                 path order; their counts scanned in that order (per 4096 tiles, exclusive_scan over those, then within)
//   emit          one workgroup per occupied tile: the tile staged in LDS in Morton order, its occupied cells ranked by wave ballots
//                 (tile_rank), key and leaf word written at the tile's offset + rank
//   levels        build_levels (device_build.hip), as the list builder ends
// For d < 4 the root cube (at most 16^3 cells) is one u-tile that is not 16-aligned in p: it is emitted as the only tile, staged from
// p = -2^d.  Every position is a prefix sum and nothing is decided by an atomic, so two calls write the same bytes.
//
// The reduce and order steps are shared with the grid editor (grid_edit.hip), whose tiles carry two counts.
//
// Export.  One lane per cell descends from the root record, following base + popc(mask & (bit(s) - 1)) as extract.hip does, so it
// reads every layout of the records.  A wave takes 64 consecutive cells of one z row: its lanes share the descent down to the last
// levels (one cache line per record for the whole wave) and its stores are 256 contiguous bytes.
#include <algorithm>
#include <climits>

#include "ctx.h"
#include "grid.h"

namespace vxrt {
namespace {

constexpr uint32_t kThreads = kTileThreads;        // one thread per 16-cell row of a tile (16 x 16 rows)
constexpr uint32_t kWaves = kTileWaves;
constexpr uint32_t kChunk = 4096;                  // sorted tiles per offset block
constexpr uint32_t kChunkItems = kChunk / kThreads;

// ---- the tile pipeline: reduce, order ------------------------------------------------------------------------------------------
// out[block] = the sums and the min / max over in[block, block + grid, ...)
__global__ __launch_bounds__(kThreads) void grid_tile_reduce_kernel(const TileStat* in, uint32_t n, TileStat* out) {
    __shared__ TileStat lds[kWaves];
    TileStat v{{0, 0}, 0, 0, {INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const TileStat t = in[i];
        v.count[0] += t.count[0];
        v.count[1] += t.count[1];
        v.active += t.active;
        for (int a = 0; a < 3; a++) { v.lo[a] = min(v.lo[a], t.lo[a]); v.hi[a] = max(v.hi[a], t.hi[a]); }
    }
    block_tile_stat(v, false, lds, out + blockIdx.x);
}

// keys[t] = tile t's path code when it is active, 2^bits (past every code) when it is not
__global__ __launch_bounds__(kThreads) void grid_tile_code_kernel(const GridDesc g, const TileStat* stats, uint32_t ntiles, uint32_t depth,
                                                                   uint32_t bits, uint64_t* keys, uint32_t* vals) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= ntiles) return;
    keys[t] = stats[t].active ? tile_code(g, t, depth) : uint64_t(1) << bits;
    vals[t] = t;
}

__global__ __launch_bounds__(kThreads) void grid_chunk_sum_kernel(const TileStat* stats, const uint32_t* order, uint32_t n, uint64_t* part) {
    __shared__ uint64_t lds[kWaves];
    uint64_t sum = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < kChunkItems; j++) {
        const uint32_t i = blockIdx.x * kChunk + j * kThreads + threadIdx.x;
        if (i < n) sum += tile_weight(stats[order[i]]);
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = 0;
        for (uint32_t w = 0; w < kWaves; w++) all += lds[w];
        part[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kThreads) void grid_chunk_offsets_kernel(const TileStat* stats, const uint32_t* order, uint32_t n,
                                                                      const uint64_t* part, uint64_t* offset) {
    __shared__ uint64_t lds[kWaves];
    uint64_t at = part[blockIdx.x];
#pragma unroll 1
    for (uint32_t j = 0; j < kChunkItems; j++) {
        const uint32_t i = blockIdx.x * kChunk + j * kThreads + threadIdx.x;
        const uint64_t c = i < n ? tile_weight(stats[order[i]]) : 0ull;
        uint64_t total;
        const uint64_t o = at + block_exclusive<uint64_t, kWaves>(c, lds, &total);
        at += total;
        if (i < n) offset[i] = o;
    }
}

// ---- the builder: tile stats, emit ---------------------------------------------------------------------------------------------
// count[0]: the tile's occupied cells; lo / hi: their bounds per axis
__global__ __launch_bounds__(kThreads) void grid_tile_stats_kernel(const GridDesc g, const uint32_t* pal, TileStat* stats) {
    __shared__ TileStat lds[kWaves];
    int p0[3];
    tile_origin(g, 0u, 0u, blockIdx.x, p0);
    const int px = p0[0] + int(threadIdx.x >> 4), py = p0[1] + int(threadIdx.x & 15u);
    uint32_t w[16];
    load_row(g, pal, px, py, p0[2], w);
    uint32_t occ = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) occ |= (w[k] >> 31) << k;
    TileStat v{{uint32_t(__popc(occ)), 0}, 0, 0, {INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}};
    if (occ) {
        v.lo[0] = v.hi[0] = px;
        v.lo[1] = v.hi[1] = py;
        v.lo[2] = p0[2] + __builtin_ctz(occ);
        v.hi[2] = p0[2] + 31 - __builtin_clz(occ);
    }
    block_tile_stat(v, true, lds, stats + blockIdx.x);
}

// Workgroup b: the b-th active tile in path order (order[b]; small: the root cube of a depth < 4 tree, the only tile).  Its cells
// are staged in LDS at their in-tile Morton index and ranked by tile_rank.
__global__ __launch_bounds__(kThreads) void grid_emit_kernel(const GridDesc g, const uint32_t* pal, const uint32_t* order,
                                                             const uint64_t* offset, uint32_t depth, uint32_t small, uint64_t m,
                                                             uint64_t* ukeys, int32_t* leaves) {
    __shared__ uint32_t s_cell[kTileCells];
    __shared__ uint32_t s_off[1][kTileRounds * kWaves];
    const uint32_t t = threadIdx.x;
    int p0[3];
    uint64_t code = 0, at = 0;
    if (small) {
        tile_origin(g, 1u, depth, 0u, p0);
    } else {
        const uint32_t tile = order[blockIdx.x];
        tile_origin(g, 0u, depth, tile, p0);
        code = tile_code(g, tile, depth);
        at = offset[blockIdx.x];
    }
    const uint32_t x = t >> 4, y = t & 15u;
    uint32_t w[16];
    load_row(g, pal, p0[0] + int(x), p0[1] + int(y), p0[2], w);
#pragma unroll
    for (uint32_t z = 0; z < 16; z++) s_cell[morton4(x, y, z)] = w[z];
    __syncthreads();
    tile_rank_scan<1>([&](uint32_t j, uint32_t) { return (s_cell[j * kThreads + t] >> 31) != 0u; }, s_off);
#pragma unroll
    for (uint32_t j = 0; j < kTileRounds; j++) {
        const uint32_t mi = j * kThreads + t;
        const uint32_t cw = s_cell[mi];
        const uint64_t o = at + tile_rank(s_off[0], j, cw >> 31);
        if ((cw >> 31) && o < m) {   // o < m unless the grid changed between the passes (a race of the caller's): then nothing past m is written
            ukeys[o] = code << 12 | mi;
            leaves[o] = int32_t(cw);
        }
    }
}

// ---- export --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grid_export_kernel(const SvoRecord* svo, const int32_t* leaves, uint32_t depth, int3 o,
                                                               uint3 n, uint32_t zsegs, uint64_t units, uint32_t* cells) {
    const uint32_t lane = threadIdx.x & 63u;
    const int64_t half = int64_t(1) << depth;
    for (uint64_t unit = uint64_t(blockIdx.x) * kWaves + (threadIdx.x >> 6); unit < units; unit += uint64_t(gridDim.x) * kWaves) {
        const uint64_t row = unit / zsegs;
        const uint32_t k = uint32_t(unit - row * zsegs) * 64u + lane;
        if (k >= n.z) continue;
        const uint32_t j = uint32_t(row % n.y);
        const uint64_t i = row / n.y;
        const int64_t u[3] = {int64_t(o.x) + int64_t(i) + half, int64_t(o.y) + int64_t(j) + half, int64_t(o.z) + int64_t(k) + half};
        uint32_t word = 0;
        if (u[0] >= 0 && u[0] < 2 * half && u[1] >= 0 && u[1] < 2 * half && u[2] >= 0 && u[2] < 2 * half)
            word = leaf_at(svo, leaves, depth, uint32_t(u[0]), uint32_t(u[1]), uint32_t(u[2]));
        cells[(i * n.y + j) * n.z + k] = word;
    }
}

}  // namespace

hipError_t launch_tile_reduce(const TileStat* stats, uint32_t n, TileStat* part, TileStat* dst, hipStream_t s) {
    hipLaunchKernelGGL(grid_tile_reduce_kernel, dim3(kTileReduceBlocks), dim3(kThreads), 0, s, stats, n, part);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    hipLaunchKernelGGL(grid_tile_reduce_kernel, dim3(1), dim3(kThreads), 0, s, part, kTileReduceBlocks, dst);
    return hipGetLastError();
}

int order_active_tiles(const GridDesc& g, const TileStat* stats, uint32_t ntiles, uint32_t active, uint32_t depth, hipStream_t s,
                       const char* who, TileOrder* out) {
    const uint32_t chunks = (active + kChunk - 1) / kChunk, bits = 3u * (depth - 3u);
    if (int rc = out->sort.alloc(ntiles, true, who, "the tile codes", "the tile codes")) return rc;
    if (int rc = alloc_scratch(&out->part, (size_t(chunks) + 1) * sizeof(uint64_t), who, "the tile offsets")) return rc;
    if (int rc = alloc_scratch(&out->offset, size_t(active) * sizeof(uint64_t), who, "the tile offsets")) return rc;
    hipLaunchKernelGGL(grid_tile_code_kernel, dim3((ntiles + kThreads - 1) / kThreads), dim3(kThreads), 0, s, g, stats, ntiles, depth, bits,
                       out->sort.keys(), out->sort.vals());
    HIP_TRY(hipGetLastError());
    HIP_TRY(out->sort.sort(ntiles, bits + 1u, s));
    out->order = out->sort.vals();
    hipLaunchKernelGGL(grid_chunk_sum_kernel, dim3(chunks), dim3(kThreads), 0, s, stats, out->order, active, out->part.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_exclusive_scan(out->part.as<uint64_t>(), chunks, s));
    hipLaunchKernelGGL(grid_chunk_offsets_kernel, dim3(chunks), dim3(kThreads), 0, s, stats, out->order, active, out->part.as<uint64_t>(),
                       out->offset.as<uint64_t>());
    HIP_TRY(hipGetLastError());
    return VXRT_OK;
}

int build_svo_device_grid(const GridDesc& g, const uint32_t* pal, hipStream_t s, DeviceTree* out) {
    const char* who = "vxrt_set_voxel_grid";
    *out = DeviceTree{};
    const uint64_t ntiles64 = uint64_t(g.nt[0]) * g.nt[1] * g.nt[2];
    if (ntiles64 >= (uint64_t(1) << 31)) { set_error("vxrt_set_voxel_grid: 2^31 tiles or more"); return VXRT_E_SCENE; }
    const uint32_t ntiles = uint32_t(ntiles64);

    // tile stats -> the occupied count and the coordinates' min / max -> the depth
    ScratchBuffer stats, red;
    if (int rc = alloc_scratch(&stats, size_t(ntiles) * sizeof(TileStat), who, "the tile counts")) return rc;
    if (int rc = alloc_scratch(&red, (kTileReduceBlocks + 1) * sizeof(TileStat), who, "the tile counts")) return rc;
    hipLaunchKernelGGL(grid_tile_stats_kernel, dim3(ntiles), dim3(kThreads), 0, s, g, pal, stats.as<TileStat>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_tile_reduce(stats.as<TileStat>(), ntiles, red.as<TileStat>(), red.as<TileStat>() + kTileReduceBlocks, s));
    TileStat all;
    HIP_TRY(hipMemcpyAsync(&all, red.as<TileStat>() + kTileReduceBlocks, sizeof all, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (all.count[0] == 0) return build_empty_tree(s, who, out);
    if (all.count[0] >= (uint64_t(1) << 32)) { set_error("vxrt_set_voxel_grid: 2^32 occupied cells or more"); return VXRT_E_SCENE; }
    const uint32_t depth = depth_of_bounds(std::min({all.lo[0], all.lo[1], all.lo[2]}), std::max({all.hi[0], all.hi[1], all.hi[2]}));
    const size_t m = size_t(all.count[0]);   // depth <= 15: the box lies in the int16 range

    ScratchBuffer ukeys, leaves, part, bins;
    TileOrder tiles;
    if (int rc = alloc_scratch(&ukeys, m * sizeof(uint64_t), who, "the keys")) return rc;
    if (int rc = alloc_scratch(&leaves, m * sizeof(int32_t), who, "the leaf words")) return rc;
    if (depth < 4u) {   // the root cube is one tile
        hipLaunchKernelGGL(grid_emit_kernel, dim3(1), dim3(kThreads), 0, s, g, pal, nullptr, nullptr, depth, 1u, uint64_t(m),
                           ukeys.as<uint64_t>(), leaves.as<int32_t>());
    } else {
        if (int rc = order_active_tiles(g, stats.as<TileStat>(), ntiles, all.active, depth, s, who, &tiles)) return rc;
        hipLaunchKernelGGL(grid_emit_kernel, dim3(all.active), dim3(kThreads), 0, s, g, pal, tiles.order, tiles.offset.as<uint64_t>(), depth,
                           0u, uint64_t(m), ukeys.as<uint64_t>(), leaves.as<int32_t>());
    }
    HIP_TRY(hipGetLastError());
    if (int rc = alloc_scratch(&part, level_part_entries(m) * sizeof(uint64_t), who, "the scan partials")) return rc;
    if (int rc = alloc_scratch(&bins, level_bin_entries(m) * sizeof(uint64_t), who, "the level counts")) return rc;
    return build_levels(ukeys.as<uint64_t>(), nullptr, m, part.as<uint64_t>(), bins.as<uint64_t>(), depth, &leaves, s, who, out);
}

hipError_t launch_grid_export(const SvoRecord* svo, const int32_t* leaves, uint32_t depth, const int32_t o[3], const uint32_t n[3],
                              uint32_t* cells, hipStream_t s) {
    const uint32_t zsegs = (n[2] + 63u) / 64u;
    const uint64_t units = uint64_t(n[0]) * n[1] * zsegs;
    const uint64_t blocks = std::min<uint64_t>((units + kWaves - 1) / kWaves, uint64_t(1) << 20);
    hipLaunchKernelGGL(grid_export_kernel, dim3(uint32_t(blocks)), dim3(kThreads), 0, s, svo, leaves, depth, make_int3(o[0], o[1], o[2]),
                       make_uint3(n[0], n[1], n[2]), zsegs, units, cells);
    return hipGetLastError();
}

}  // namespace vxrt
