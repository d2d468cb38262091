// grid.h — what api_grid.hip (host side of vxrt_grid.h), grid_build.hip (its kernels) and grid_edit.hip (vxrt_grid_edit.h) share:
// the grid, and the tile pipeline both run over its 16-aligned tiles (grid_build.hip).  DESIGN.md §12, §13.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "block_scan.h"
#include "device_build.h"

namespace vxrt {

// A dense grid of cells in device memory, C order [x][y][z] (z fastest): cell (i, j, k) is the voxel position o + (i, j, k).
// format 1: uint8 palette indices (0 empty); 2: uint32 cells (bit 31 set: the cell is the leaf word; clear: empty).
struct GridDesc {
    const void* cells;
    uint32_t format;
    int32_t o[3];      // origin
    uint32_t n[3];     // dims, each >= 1
    int32_t t0[3];     // the first 16-aligned tile per axis: floor(o / 16)
    uint32_t nt[3];    // tiles per axis
};

// ---- device helpers of the grid kernels (grid_build.hip, grid_edit.hip) -------------------------------------------------------
// 4 bits per axis, x highest: bit k of x -> bit 3k + 2, of y -> 3k + 1, of z -> 3k
__device__ __forceinline__ uint32_t morton4(uint32_t x, uint32_t y, uint32_t z) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) m |= ((x >> k) & 1u) << (3u * k + 2u) | ((y >> k) & 1u) << (3u * k + 1u) | ((z >> k) & 1u) << (3u * k);
    return m;
}

__device__ __forceinline__ uint64_t morton_tile(uint32_t x, uint32_t y, uint32_t z, uint32_t bits) {
    uint64_t m = 0;
    for (uint32_t k = 0; k < bits; k++)
        m |= uint64_t(((x >> k) & 1u) << 2 | ((y >> k) & 1u) << 1 | ((z >> k) & 1u)) << (3u * k);
    return m;
}

// The 16 cells p = (px, py, pz0 .. pz0 + 15) as leaf words (0: empty or outside the grid's box; the box may be any int32 box).  A row wholly inside the box whose
// address is 16-byte aligned is read with 16-byte loads (one for uint8 cells, four for uint32 cells).
__device__ __forceinline__ void load_row(const GridDesc& g, const uint32_t* pal, int px, int py, int pz0, uint32_t w[16]) {
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = 0u;
    const int64_t i = int64_t(px) - g.o[0], j = int64_t(py) - g.o[1], k0 = int64_t(pz0) - g.o[2], n2 = g.n[2];
    if (i < 0 || i >= int64_t(g.n[0]) || j < 0 || j >= int64_t(g.n[1])) return;
    const size_t row = (size_t(i) * g.n[1] + size_t(j)) * g.n[2];
    const bool whole = k0 >= 0 && k0 + 16 <= n2;
    if (g.format == 1u) {
        const uint8_t* q = static_cast<const uint8_t*>(g.cells) + row;
        if (whole && (reinterpret_cast<uintptr_t>(q + k0) & 15u) == 0u) {
            const uint4 v = *reinterpret_cast<const uint4*>(q + k0);
            const uint32_t b[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++) w[k] = pal[(b[k >> 2] >> (8 * (k & 3))) & 0xffu];
            return;
        }
#pragma unroll
        for (int k = 0; k < 16; k++)
            if (k0 + k >= 0 && k0 + k < n2) w[k] = pal[q[k0 + k]];
    } else {
        const uint32_t* q = static_cast<const uint32_t*>(g.cells) + row;
        if (whole && (reinterpret_cast<uintptr_t>(q + k0) & 15u) == 0u) {
#pragma unroll
            for (int v4 = 0; v4 < 4; v4++) {
                const uint4 v = reinterpret_cast<const uint4*>(q + k0)[v4];
                w[4 * v4 + 0] = v.x; w[4 * v4 + 1] = v.y; w[4 * v4 + 2] = v.z; w[4 * v4 + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (k0 + k >= 0 && k0 + k < n2) w[k] = q[k0 + k];
        }
#pragma unroll
        for (int k = 0; k < 16; k++) w[k] = w[k] >> 31 ? w[k] : 0u;
    }
}

__device__ __forceinline__ void tile_coords(const GridDesc& g, uint32_t tile, int* tx, int* ty, int* tz) {
    *tz = g.t0[2] + int(tile % g.nt[2]);
    const uint32_t r = tile / g.nt[2];
    *ty = g.t0[1] + int(r % g.nt[1]);
    *tx = g.t0[0] + int(r / g.nt[1]);
}

// The first cell of tile `tile`; small: the root cube of a depth < 4 tree, the only tile, from p = -2^depth (not 16-aligned).
__device__ __forceinline__ void tile_origin(const GridDesc& g, uint32_t small, uint32_t depth, uint32_t tile, int p0[3]) {
    if (small) {
        p0[0] = p0[1] = p0[2] = -(1 << depth);
    } else {
        tile_coords(g, tile, &p0[0], &p0[1], &p0[2]);
        for (int a = 0; a < 3; a++) p0[a] *= 16;
    }
}

// The path code of tile `tile` (depth >= 4): the Morton code of its u-tile (p-tile + 2^(depth - 4) per axis), 3 (depth - 3) bits.
// A cell's path key is this << 12 | its in-tile Morton index.
__device__ __forceinline__ uint64_t tile_code(const GridDesc& g, uint32_t tile, uint32_t depth) {
    int tx, ty, tz;
    tile_coords(g, tile, &tx, &ty, &tz);
    const int shift = 1 << (depth - 4u);
    return morton_tile(uint32_t(tx + shift), uint32_t(ty + shift), uint32_t(tz + shift), depth - 3u);
}

// ---- the tile pipeline (grid_build.hip: the builder; grid_edit.hip: the editor) -----------------------------------------------
//   summary   one workgroup per tile, one thread per 16-cell row: a TileStat per tile -> launch_tile_reduce -> one read-back
//   order     order_active_tiles: the active tiles in path order and their offsets
//   emit      one workgroup per active tile: the tile staged in LDS in Morton order, its cells ranked by tile_rank_scan / tile_rank
constexpr uint32_t kTileThreads = 256;
constexpr uint32_t kTileWaves = kTileThreads / 64;
constexpr uint32_t kTileCells = 4096;
constexpr uint32_t kTileRounds = kTileCells / kTileThreads;
constexpr uint32_t kTileReduceBlocks = 1024;

// A tile's summary: two counts (the builder: its occupied cells, 0; the editor: its clears, its sets), whether it has a cell to emit
// and the least and greatest position per axis of its occupied cells (the editor: of its sets).  Reduced: the sums, the number of
// active tiles, the bounds.
struct TileStat {
    uint64_t count[2];
    uint32_t active;
    uint32_t pad;
    int32_t lo[3], hi[3];
};

// a tile's weight in the scan of the active tiles: count[0] low, count[1] high (either total < 2^32, so the sums never carry)
__device__ __forceinline__ uint64_t tile_weight(const TileStat& t) { return t.count[0] | t.count[1] << 32; }

// The sums and bounds of the block's v -> *dst (thread 0).  tile: v is a thread's share of one tile, and dst->active is whether the
// tile has a count; else dst->active is the sum of v.active.  lds: kTileWaves entries.
__device__ __forceinline__ void block_tile_stat(TileStat v, bool tile, TileStat* lds, TileStat* dst) {
    v.count[0] = wave_sum(v.count[0]);
    v.count[1] = wave_sum(v.count[1]);
    v.active = wave_sum(v.active);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (int a = 0; a < 3; a++) {
            v.lo[a] = min(v.lo[a], __shfl_xor(v.lo[a], off, 64));
            v.hi[a] = max(v.hi[a], __shfl_xor(v.hi[a], off, 64));
        }
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kTileWaves; w++) {
            v.count[0] += lds[w].count[0];
            v.count[1] += lds[w].count[1];
            v.active += lds[w].active;
            for (int a = 0; a < 3; a++) { v.lo[a] = min(v.lo[a], lds[w].lo[a]); v.hi[a] = max(v.hi[a], lds[w].hi[a]); }
        }
        if (tile) v.active = v.count[0] + v.count[1] != 0u ? 1u : 0u;
        *dst = v;
    }
}

// In-tile ranking.  With the tile staged in LDS at the in-tile Morton index, thread 64 wave + lane takes cell 256 j + 64 wave + lane
// in round j.  tile_rank_scan: off[k][4 j + wave] = the cells of list k (flag(j, k)) before round j's wave, one ballot per
// (round, wave) and one wave-wide scan of the 64 counts per list.  tile_rank: a flagged cell's rank in its list.
template <uint32_t N, typename Flag> __device__ __forceinline__ void tile_rank_scan(Flag flag, uint32_t (*off)[kTileRounds * kTileWaves]) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t j = 0; j < kTileRounds; j++)
#pragma unroll
        for (uint32_t k = 0; k < N; k++) {
            const uint64_t b = __ballot(flag(j, k));
            if (lane == 0u) off[k][j * kTileWaves + wave] = uint32_t(__popcll(b));
        }
    __syncthreads();
    if (wave == 0u)
#pragma unroll
        for (uint32_t k = 0; k < N; k++) {
            const uint32_t c = off[k][lane];
            off[k][lane] = wave_inclusive(c, lane) - c;
        }
    __syncthreads();
}

__device__ __forceinline__ uint32_t tile_rank(const uint32_t* off, uint32_t j, bool flag) {
    return off[j * kTileWaves + (threadIdx.x >> 6)] + lanes_below(__ballot(flag));
}

// The leaf word of the voxel at u = p + 2^depth (u inside the root cube [0, 2^(depth+1))^3), 0 where there is none: the descent from
// the root record along base + popc(mask & (bit(s) - 1)), as extract.hip walks, so it reads every layout of the 8-byte records.
__device__ __forceinline__ uint32_t leaf_at(const SvoRecord* svo, const int32_t* leaves, uint32_t depth, uint32_t ux, uint32_t uy,
                                            uint32_t uz) {
    uint32_t node = 0;
    for (uint32_t l = 0; l <= depth; l++) {
        const uint2 r = *reinterpret_cast<const uint2*>(svo + node);
        const uint32_t b = depth - l;
        const uint32_t s = ((ux >> b) & 1u) << 2 | ((uy >> b) & 1u) << 1 | ((uz >> b) & 1u);
        const uint32_t mask = l == depth ? (r.x >> 8) & 0xffu : r.x & 0xffu;
        if (!((mask >> s) & 1u)) return 0u;
        const uint32_t slot = r.y + uint32_t(__popc(mask & ((1u << s) - 1u)));
        if (l == depth) return uint32_t(leaves[slot]);
        node = slot;
    }
    return 0u;
}

// stats[0 .. n) reduced to *dst on `stream` (two launches); part: kTileReduceBlocks entries.
hipError_t launch_tile_reduce(const TileStat* stats, uint32_t n, TileStat* part, TileStat* dst, hipStream_t stream);

// The `active` active tiles of g's ntiles in path order (depth >= 4), enqueued on `stream`: the tiles keyed by tile_code, inactive
// ones past every code, sorted (KeySort); then their weights scanned in that order.  order[0 .. active): their indices,
// offset[0 .. active): the exclusive prefix sums of their weights.  The buffers live as long as *out.  who: the API call.
struct TileOrder {
    KeySort sort;
    ScratchBuffer part, offset;
    const uint32_t* order = nullptr;
};
int order_active_tiles(const GridDesc& g, const TileStat* stats, uint32_t ntiles, uint32_t active, uint32_t depth, hipStream_t stream,
                       const char* who, TileOrder* out);

// The scene of the grid's occupied cells, exactly as build_svo_device_list builds it from them as a list.  pal: for format 1, 256
// leaf words in device memory (entry 0 = 0).  The grid is read on `stream` behind what is enqueued there; waits for the result.
// VXRT_E_SCENE: 2^32 occupied cells or more, or 2^32 records or more; VXRT_E_DEVICE: an allocation failed.  Nothing is allocated on
// failure.
int build_svo_device_grid(const GridDesc& g, const uint32_t* pal, hipStream_t stream, DeviceTree* out);

// Enqueues on `stream`: cells[(i * n1 + j) * n2 + k] = the leaf word of the voxel at o + (i, j, k), 0 where there is none (outside
// the root cube [-2^depth, 2^depth)^3 included).  n0 * n1 * n2 > 0.
hipError_t launch_grid_export(const SvoRecord* svo, const int32_t* leaves, uint32_t depth, const int32_t o[3], const uint32_t n[3],
                              uint32_t* cells, hipStream_t stream);

}  // namespace vxrt
