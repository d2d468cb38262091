// grid_build.hip — device side of vxrt_grid.h: a scene built from a dense grid of cells (vxrt_set_voxel_grid), and a box of the scene
// written back as a dense grid of leaf words (vxrt_get_voxel_grid).  The host side is api_grid.hip; DESIGN.md §12.
//
// Import.  With d the depth and u = p + 2^d, a 16-aligned tile of p is a 16-aligned tile of u whenever d >= 4 (2^d is a multiple of
// 16), and a voxel's path key is (the Morton code of its u-tile) << 12 | (the Morton code of its cell in the tile).  So the occupied
// cells, taken tile by tile in ascending tile code and in Morton order inside each tile, are already the sorted, unique key list the
// list builder makes with its radix sort and dedupe (device_build.hip); only the tiles need sorting, about one per 4096 cells.
//   tile stats    one workgroup per 16-aligned tile of the grid's box: its occupied count and the min / max of its occupied cells'
//                 coordinates (every axis together: build_octree's depth rule needs no more) -> reduced -> the depth, the total
//   tile codes    per tile: the Morton code of its u-tile (d >= 4) -> radix_sort_pairs (3(d - 3) bits) -> the tiles in path order
//   offsets       the sorted tiles' counts, scanned (per 4096 tiles, extract_scan over those, then within): every tile's first key
//   emit          one workgroup per sorted tile: the tile staged in LDS in Morton order, its occupied cells ranked by wave ballots,
//                 key and leaf word written at the tile's offset + rank
//   levels        build_levels (device_build.hip), as the list builder ends
// For d < 4 the root cube (at most 16^3 cells) is one u-tile that is not 16-aligned in p: it is emitted as the only tile, staged from
// p = -2^d.  Every position is a prefix sum and nothing is decided by an atomic, so two calls write the same bytes.
//
// Export.  One lane per cell descends from the root record, following base + popc(mask & (bit(s) - 1)) as extract.hip does, so it
// reads every layout of the records.  A wave takes 64 consecutive cells of one z row: its lanes share the descent down to the last
// levels (one cache line per record for the whole wave) and its stores are 256 contiguous bytes.
#include <algorithm>
#include <climits>
#include <string>

#include "block_scan.h"
#include "ctx.h"
#include "extract.h"
#include "grid.h"

namespace vxrt {
namespace {

constexpr uint32_t kThreads = 256;                 // one thread per 16-cell row of a tile (16 x 16 rows)
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kTileCells = 4096;
constexpr uint32_t kChunk = 4096;                  // sorted tiles per offset block
constexpr uint32_t kChunkItems = kChunk / kThreads;
constexpr uint32_t kReduceBlocks = 1024;

struct Stat {
    uint64_t count;
    int lo, hi;
};

// ---- tile stats ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void grid_tile_stats_kernel(const GridDesc g, const uint32_t* pal, Stat* stats) {
    __shared__ uint32_t s_cnt[kWaves];
    __shared__ int s_lo[kWaves], s_hi[kWaves];
    int tx, ty, tz;
    tile_coords(g, blockIdx.x, &tx, &ty, &tz);
    const int px = tx * 16 + int(threadIdx.x >> 4), py = ty * 16 + int(threadIdx.x & 15u), pz0 = tz * 16;
    uint32_t w[16];
    load_row(g, pal, px, py, pz0, w);
    uint32_t cnt = 0;
    int zlo = INT_MAX, zhi = INT_MIN;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        if (w[k] >> 31) {
            cnt++;
            zlo = min(zlo, pz0 + k);
            zhi = max(zhi, pz0 + k);
        }
    }
    int lo = INT_MAX, hi = INT_MIN;
    if (cnt) { lo = min(min(px, py), zlo); hi = max(max(px, py), zhi); }
    cnt = wave_sum(cnt);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63u) == 0u) { s_cnt[threadIdx.x >> 6] = cnt; s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t v = 1; v < kWaves; v++) { cnt += s_cnt[v]; lo = min(lo, s_lo[v]); hi = max(hi, s_hi[v]); }
        stats[blockIdx.x] = Stat{cnt, lo, hi};
    }
}

// out[block] = the sum of counts and the min / max over in[block, block + grid, ...)
__global__ __launch_bounds__(kThreads) void grid_stat_reduce_kernel(const Stat* in, uint32_t n, Stat* out) {
    __shared__ uint64_t s_cnt[kWaves];
    __shared__ int s_lo[kWaves], s_hi[kWaves];
    uint64_t cnt = 0;
    int lo = INT_MAX, hi = INT_MIN;
    for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
        const Stat t = in[i];
        cnt += t.count;
        lo = min(lo, t.lo);
        hi = max(hi, t.hi);
    }
    cnt = wave_sum(cnt);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63u) == 0u) { s_cnt[threadIdx.x >> 6] = cnt; s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t v = 1; v < kWaves; v++) { cnt += s_cnt[v]; lo = min(lo, s_lo[v]); hi = max(hi, s_hi[v]); }
        out[blockIdx.x] = Stat{cnt, lo, hi};
    }
}

// ---- tile codes and offsets ----------------------------------------------------------------------------------------------------
// keys[t] = the Morton code of tile t's u-tile (p-tile + 2^(depth - 4) per axis), 0 for an empty tile (it emits nothing)
__global__ __launch_bounds__(kThreads) void grid_tile_code_kernel(const GridDesc g, const Stat* stats, uint32_t ntiles, uint32_t depth,
                                                                   uint64_t* keys, uint32_t* vals) {
    const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= ntiles) return;
    uint64_t key = 0;
    if (stats[t].count) {
        int tx, ty, tz;
        tile_coords(g, t, &tx, &ty, &tz);
        const int shift = 1 << (depth - 4u);
        key = morton_tile(uint32_t(tx + shift), uint32_t(ty + shift), uint32_t(tz + shift), depth - 3u);
    }
    keys[t] = key;
    vals[t] = t;
}

__global__ __launch_bounds__(kThreads) void grid_chunk_sum_kernel(const Stat* stats, const uint32_t* order, uint32_t ntiles, uint64_t* part) {
    __shared__ uint64_t lds[kWaves];
    uint64_t sum = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < kChunkItems; j++) {
        const uint32_t i = blockIdx.x * kChunk + j * kThreads + threadIdx.x;
        if (i < ntiles) sum += stats[order[i]].count;
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

__global__ __launch_bounds__(kThreads) void grid_chunk_offsets_kernel(const Stat* stats, const uint32_t* order, uint32_t ntiles,
                                                                      const uint64_t* part, uint64_t* offset) {
    __shared__ uint64_t lds[kWaves];
    uint64_t at = part[blockIdx.x];
#pragma unroll 1
    for (uint32_t j = 0; j < kChunkItems; j++) {
        const uint32_t i = blockIdx.x * kChunk + j * kThreads + threadIdx.x;
        const uint64_t c = i < ntiles ? stats[order[i]].count : 0ull;
        uint64_t total;
        const uint64_t o = at + block_exclusive<uint64_t, kWaves>(c, lds, &total);
        at += total;
        if (i < ntiles) offset[i] = o;
    }
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------
// Workgroup b: the b-th tile in path order (order[b]; small: the root cube of a depth < 4 tree, the only tile).  Its cells are staged in
// LDS at their in-tile Morton index m; cell m = 256 j + 64 wave + lane is ranked in round j by the wave's ballot, the rounds and
// waves in that order by one wave-wide scan of the 64 (round, wave) counts.
__global__ __launch_bounds__(kThreads) void grid_emit_kernel(const GridDesc g, const uint32_t* pal, const Stat* stats, const uint32_t* order,
                                                             const uint64_t* offset, uint32_t depth, uint32_t small, uint64_t m,
                                                             uint64_t* ukeys, int32_t* leaves) {
    __shared__ uint32_t s_cell[kTileCells];
    __shared__ uint32_t s_off[kTileCells / 64];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    int p0[3];
    uint64_t code = 0, at = 0;
    if (small) {
        p0[0] = p0[1] = p0[2] = -(1 << depth);
    } else {
        const uint32_t tile = order[blockIdx.x];
        if (stats[tile].count == 0) return;
        int tc[3];
        tile_coords(g, tile, &tc[0], &tc[1], &tc[2]);
        const int shift = 1 << (depth - 4u);
        for (int a = 0; a < 3; a++) p0[a] = tc[a] * 16;
        code = morton_tile(uint32_t(tc[0] + shift), uint32_t(tc[1] + shift), uint32_t(tc[2] + shift), depth - 3u);
        at = offset[blockIdx.x];
    }
    const uint32_t x = t >> 4, y = t & 15u;
    uint32_t w[16];
    load_row(g, pal, p0[0] + int(x), p0[1] + int(y), p0[2], w);
#pragma unroll
    for (uint32_t z = 0; z < 16; z++) s_cell[morton4(x, y, z)] = w[z];
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kTileCells / kThreads; j++) {
        const uint64_t occ = __ballot(s_cell[j * kThreads + t] >> 31);
        if (lane == 0u) s_off[j * kWaves + wave] = uint32_t(__popcll(occ));
    }
    __syncthreads();
    if (wave == 0u) {
        const uint32_t c = s_off[lane];
        s_off[lane] = wave_inclusive(c, lane) - c;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t j = 0; j < kTileCells / kThreads; j++) {
        const uint32_t mi = j * kThreads + t;
        const uint32_t cw = s_cell[mi];
        const uint64_t occ = __ballot(cw >> 31);
        if (cw >> 31) {   // o < m unless the grid changed between the passes (a race of the caller's): then nothing past m is written
            const uint64_t o = at + s_off[j * kWaves + wave] +
                               __builtin_amdgcn_mbcnt_hi(uint32_t(occ >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(occ), 0u));
            if (o < m) {
                ukeys[o] = code << 12 | mi;
                leaves[o] = int32_t(cw);
            }
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

hipError_t alloc(ScratchBuffer* b, size_t bytes, size_t* total) {
    *total += bytes;
    const hipError_t e = b->alloc(bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); b->p = nullptr; }
    return e;
}

int fail(hipError_t e, const char* what) {
    set_error(std::string("vxrt_set_voxel_grid: allocating ") + what + ": " + hipGetErrorString(e));
    return VXRT_E_DEVICE;
}

}  // namespace

int build_svo_device_grid(const GridDesc& g, const uint32_t* pal, hipStream_t s, DeviceTree* out) {
    *out = DeviceTree{};
    const uint64_t ntiles64 = uint64_t(g.nt[0]) * g.nt[1] * g.nt[2];
    if (ntiles64 >= (uint64_t(1) << 31)) { set_error("vxrt_set_voxel_grid: 2^31 tiles or more"); return VXRT_E_SCENE; }
    const uint32_t ntiles = uint32_t(ntiles64);
    size_t scratch = 0;

    // tile stats -> the occupied count and the coordinates' min / max -> the depth
    ScratchBuffer stats, red;
    if (hipError_t e = alloc(&stats, size_t(ntiles) * sizeof(Stat), &scratch); e != hipSuccess) return fail(e, "the tile counts");
    if (hipError_t e = alloc(&red, (kReduceBlocks + 1) * sizeof(Stat), &scratch); e != hipSuccess) return fail(e, "the tile counts");
    hipLaunchKernelGGL(grid_tile_stats_kernel, dim3(ntiles), dim3(kThreads), 0, s, g, pal, stats.as<Stat>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(grid_stat_reduce_kernel, dim3(kReduceBlocks), dim3(kThreads), 0, s, stats.as<Stat>(), ntiles, red.as<Stat>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(grid_stat_reduce_kernel, dim3(1), dim3(kThreads), 0, s, red.as<Stat>(), kReduceBlocks, red.as<Stat>() + kReduceBlocks);
    HIP_TRY(hipGetLastError());
    Stat all;
    HIP_TRY(hipMemcpyAsync(&all, red.as<Stat>() + kReduceBlocks, sizeof all, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (all.count == 0) return build_empty_tree(s, "vxrt_set_voxel_grid", out);
    if (all.count >= (uint64_t(1) << 32)) { set_error("vxrt_set_voxel_grid: 2^32 occupied cells or more"); return VXRT_E_SCENE; }
    const uint32_t depth = depth_of_bounds(all.lo, all.hi);   // <= 15: the box lies in the int16 range
    const size_t m = size_t(all.count);

    ScratchBuffer ukeys, leaves, keys[2], vals[2], hist, totals, cpart, offset, part, bins;
    if (hipError_t e = alloc(&ukeys, m * sizeof(uint64_t), &scratch); e != hipSuccess) return fail(e, "the keys");
    size_t outputs = 0;
    if (hipError_t e = alloc(&leaves, m * sizeof(int32_t), &outputs); e != hipSuccess) return fail(e, "the leaf words");
    if (depth < 4u) {   // the root cube is one tile
        hipLaunchKernelGGL(grid_emit_kernel, dim3(1), dim3(kThreads), 0, s, g, pal, stats.as<Stat>(), nullptr, nullptr, depth, 1u, uint64_t(m),
                           ukeys.as<uint64_t>(), leaves.as<int32_t>());
        HIP_TRY(hipGetLastError());
    } else {
        // the tiles in path order: their codes sorted, then their counts scanned in that order
        for (int b = 0; b < 2; b++) {
            if (hipError_t e = alloc(&keys[b], size_t(ntiles) * sizeof(uint64_t), &scratch); e != hipSuccess) return fail(e, "the tile codes");
            if (hipError_t e = alloc(&vals[b], size_t(ntiles) * sizeof(uint32_t), &scratch); e != hipSuccess) return fail(e, "the tile codes");
        }
        const uint32_t chunks = (ntiles + kChunk - 1) / kChunk;
        if (hipError_t e = alloc(&hist, radix_hist_entries(ntiles) * sizeof(uint32_t), &scratch); e != hipSuccess) return fail(e, "the digit counts");
        if (hipError_t e = alloc(&totals, 256 * sizeof(uint32_t), &scratch); e != hipSuccess) return fail(e, "the digit counts");
        if (hipError_t e = alloc(&cpart, (size_t(chunks) + 1) * sizeof(uint64_t), &scratch); e != hipSuccess) return fail(e, "the tile offsets");
        if (hipError_t e = alloc(&offset, size_t(ntiles) * sizeof(uint64_t), &scratch); e != hipSuccess) return fail(e, "the tile offsets");
        hipLaunchKernelGGL(grid_tile_code_kernel, dim3((ntiles + kThreads - 1) / kThreads), dim3(kThreads), 0, s, g, stats.as<Stat>(), ntiles,
                           depth, keys[0].as<uint64_t>(), vals[0].as<uint32_t>());
        HIP_TRY(hipGetLastError());
        uint64_t* kp[2] = {keys[0].as<uint64_t>(), keys[1].as<uint64_t>()};
        uint32_t* vp[2] = {vals[0].as<uint32_t>(), vals[1].as<uint32_t>()};
        int cur = 0;
        HIP_TRY(radix_sort_pairs(kp, vp, ntiles, 3u * (depth - 3u), hist.as<uint32_t>(), totals.as<uint32_t>(), s, &cur));
        const uint32_t* order = vp[cur];
        hipLaunchKernelGGL(grid_chunk_sum_kernel, dim3(chunks), dim3(kThreads), 0, s, stats.as<Stat>(), order, ntiles, cpart.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(launch_extract_scan(cpart.as<uint64_t>(), chunks, s));
        hipLaunchKernelGGL(grid_chunk_offsets_kernel, dim3(chunks), dim3(kThreads), 0, s, stats.as<Stat>(), order, ntiles, cpart.as<uint64_t>(),
                           offset.as<uint64_t>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(grid_emit_kernel, dim3(ntiles), dim3(kThreads), 0, s, g, pal, stats.as<Stat>(), order, offset.as<uint64_t>(),
                           depth, 0u, uint64_t(m), ukeys.as<uint64_t>(), leaves.as<int32_t>());
        HIP_TRY(hipGetLastError());
    }
    if (hipError_t e = alloc(&part, level_part_entries(m) * sizeof(uint64_t), &scratch); e != hipSuccess) return fail(e, "the scan partials");
    if (hipError_t e = alloc(&bins, level_bin_entries(m) * sizeof(uint64_t), &scratch); e != hipSuccess) return fail(e, "the level counts");
    return build_levels(ukeys.as<uint64_t>(), nullptr, m, part.as<uint64_t>(), bins.as<uint64_t>(), depth, &leaves, scratch, s,
                        "vxrt_set_voxel_grid", out);
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
