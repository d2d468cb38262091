// morph.hip — device side of vxrt_morph.h: the neighbour mask of every voxel of a sorted unique key array (morph_mask_kernel), the
// two writes behind it (morph_keep_kernel for ERODE, morph_offer_kernel for DILATE); the first offer of each new cell is a run
// head among the sorted offers (run_heads.hip).  The host side is api_morph.hip; the offset table, the neighbour key, the two lookups and the ops' reading
// of a mask are morph_rule.h's, the kernels' contracts are in morph.h and the argument in DESIGN.md §25.
//
// Unique result: every word written is a function of the key array, its words and the connectivity alone; the counts are integer
// sums in thread order.  Bounds: every loop runs a fixed count (kMorphItems items, at most kMorphRows rows, kMorphTileSteps steps
// in the tile, at most 32 in the whole array); no workgroup waits for another, and there is no atomic.
#include "block_scan.h"
#include "morph.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kMorphThreads / 64;

// A block takes the voxels [base, base + count), base = kMorphSpan * blockIdx.x.
//  1. It stages their keys in LDS, kMorphNoKey behind the last: element e is loaded by thread e % 256 in round e / 256 — coalesced,
//     every load unconditional from a clamped index, all of a thread's loads issued before its first wait — and stays in that
//     thread's registers as one of its kMorphItems voxels.
//  2. Row by row (the row is uniform over the grid, so the offset comes through scalar registers) each thread steps its voxels'
//     keys to the neighbours' and looks all of them up in the tile: kMorphItems independent walks of kMorphTileSteps LDS reads.
//     Path order keeps most neighbours inside [first, last] of the tile, where the tile decides.
//  3. A neighbour outside that range is looked up in the whole array.  The wave takes that walk only when one of its lanes has
//     such a neighbour (a ballot: a uniform branch), and then every lane takes it, those with nothing to ask from clamped
//     indices whose answers a select drops: no load sits behind a divergent branch.
// kTile == false skips 1's LDS stores and 2 and sends every neighbour through 3.  That is the route the product takes: on the lists
// measured it was the faster one; kTile == true stays for the measurement and is tested for the same bytes.
template <bool kTile>
__global__ __launch_bounds__(kMorphThreads) void morph_mask_kernel(const MorphSet s, const uint32_t c, const uint32_t op, const uint32_t steps,
                                                                    uint32_t* __restrict__ masks, uint64_t* __restrict__ part) {
    __shared__ uint64_t tile[kMorphSpan];
    const uint32_t base = blockIdx.x * kMorphSpan;
    const uint32_t count = s.m - base > kMorphSpan ? kMorphSpan : s.m - base;
    uint64_t key[kMorphItems];
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) key[k] = s.keys[morph_safe_index(base + k * kMorphThreads + threadIdx.x, s.m)];
    uint64_t first = 0, last = 0;
    if (kTile) {
#pragma unroll
        for (uint32_t k = 0; k < kMorphItems; k++) {
            const uint32_t e = k * kMorphThreads + threadIdx.x;
            tile[e] = e < count ? key[k] : kMorphNoKey;
        }
        __syncthreads();
        first = tile[0];
        last = tile[count - 1u];
    }

    uint32_t mask[kMorphItems];
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) mask[k] = 0u;
#pragma unroll 1
    for (uint32_t r = 0; r < c; r++) {
        uint64_t q[kMorphItems];
        uint32_t at[kMorphItems];
        uint32_t fine = 0, found = 0, ask = 0;      // bit k: item k's neighbour is in range / is in the set / is asked for in the whole array
#pragma unroll
        for (uint32_t k = 0; k < kMorphItems; k++) {
            bool ok;
            asm volatile("" : "+v"(key[k]));      // keeps the three axes' parts of every key from being held across the rows: 48 VGPRs
            q[k] = neighbour_key(key[k], r, &ok);
            fine |= (ok ? 1u : 0u) << k;
            at[k] = 0u;
        }
        uint64_t probed[kMorphItems];
        if (kTile) {
#pragma unroll
            for (uint32_t step = kMorphSpan >> 1; step != 0u; step >>= 1) {
#pragma unroll
                for (uint32_t k = 0; k < kMorphItems; k++) probed[k] = tile[walk_probe(at[k], step)];
                __builtin_amdgcn_sched_barrier(0);      // all eight reads are out before the first is waited for
#pragma unroll
                for (uint32_t k = 0; k < kMorphItems; k++) at[k] = walk_take(probed[k], q[k], at[k], step, true);
            }
#pragma unroll
            for (uint32_t k = 0; k < kMorphItems; k++) probed[k] = tile[at[k]];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (uint32_t k = 0; k < kMorphItems; k++) {
                const bool inside = tile_decides(q[k], first, last);
                found |= (((probed[k] == q[k]) & inside) ? 1u : 0u) << k;
                ask |= (inside ? 0u : 1u) << k;
                at[k] = 0u;
            }
            ask &= fine;
        } else {
            ask = fine;
        }
        if (__ballot(ask != 0u) != 0ull) {      // uniform over the wave
#pragma unroll 1
            for (uint32_t left = steps; left != 0u; left--) {
                const uint64_t step = uint64_t(1) << (left - 1u);
#pragma unroll
                for (uint32_t k = 0; k < kMorphItems; k++) probed[k] = s.keys[list_index(walk_probe(at[k], step), s.m)];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (uint32_t k = 0; k < kMorphItems; k++)
                    at[k] = walk_take(probed[k], q[k], at[k], step, ((ask >> k & 1u) != 0u) & list_there(walk_probe(at[k], step), s.m));
            }
#pragma unroll
            for (uint32_t k = 0; k < kMorphItems; k++) probed[k] = s.keys[list_index(at[k], s.m)];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (uint32_t k = 0; k < kMorphItems; k++) found |= ((((ask >> k & 1u) != 0u) & (probed[k] == q[k])) ? 1u : 0u) << k;
        }
        found &= fine;
#pragma unroll
        for (uint32_t k = 0; k < kMorphItems; k++) mask[k] |= (found >> k & 1u) << r;
    }

    uint32_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint32_t e = k * kMorphThreads + threadIdx.x;
        if (e < count) {
            masks[base + e] = mask[k];
            mine += op == kMorphErode ? (keep_eroded(mask[k], c) ? 1u : 0u) : uint32_t(__builtin_popcount(offer_rows(key[k], mask[k], c)));
        }
    }
    block_sum_to<kWaves>(mine, part + blockIdx.x);
}

// The writes take a thread's items side by side (voxel base + 8 t + k), so that a block's output is in the order of its input.
// Every load is unconditional from a clamped index.
struct Items {
    uint64_t key[kMorphItems];
    uint32_t word[kMorphItems], mask[kMorphItems], live;
};

__device__ __forceinline__ Items load_items(const MorphSet& s, const uint32_t* masks) {
    Items it;
    const uint32_t at = blockIdx.x * kMorphSpan + threadIdx.x * kMorphItems;
    it.live = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint32_t i = morph_safe_index(at + k, s.m);
        it.key[k] = s.keys[i];
        it.mask[k] = masks[i];
        it.word[k] = s.words != nullptr ? s.words[i] : 0u;      // uniform over the grid
        it.live |= (at + k < s.m ? 1u : 0u) << k;
    }
    return it;
}

__global__ __launch_bounds__(kMorphThreads) void morph_keep_kernel(const MorphSet s, const uint32_t c, const uint32_t* __restrict__ masks,
                                                                   const uint64_t* __restrict__ part, uint64_t* __restrict__ out_keys,
                                                                   uint32_t* __restrict__ out_words) {
    const Items it = load_items(s, masks);
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) kept |= ((it.live >> k & 1u) != 0u && keep_eroded(it.mask[k], c) ? 1u : 0u) << k;
    block_compact<kWaves, kMorphItems, true>(kept, part, [&](uint32_t k, uint64_t to) {
        out_keys[to] = it.key[k];
        if (out_words != nullptr) out_words[to] = it.word[k];
    });
}

__global__ __launch_bounds__(kMorphThreads) void morph_offer_kernel(const MorphSet s, const uint32_t c, const uint32_t* __restrict__ masks,
                                                                    const uint64_t* __restrict__ part, uint64_t* __restrict__ out_offers,
                                                                    uint32_t* __restrict__ out_words) {
    const Items it = load_items(s, masks);
    uint32_t rows[kMorphItems], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        rows[k] = (it.live >> k & 1u) != 0u ? offer_rows(it.key[k], it.mask[k], c) : 0u;
        mine += uint32_t(__builtin_popcount(rows[k]));
    }
    __shared__ uint32_t scan[kWaves];
    uint32_t all;
    uint64_t to = part[blockIdx.x] + block_exclusive<uint32_t, kWaves>(mine, scan, &all);
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
#pragma unroll 1
        for (uint32_t r = 0; r < c; r++) {
            if (rows[k] >> r & 1u) {
                bool ok;
                out_offers[to] = offer_key(neighbour_key(it.key[k], r, &ok), r);
                if (out_words != nullptr) out_words[to] = it.word[k];
                to++;
            }
        }
    }
}

}  // namespace

hipError_t launch_morph_mask(const MorphSet& s, uint32_t c, uint32_t op, bool tile, uint32_t* masks, uint64_t* part, hipStream_t stream) {
    const dim3 grid(morph_blocks(s.m)), block(kMorphThreads);
    const uint32_t steps = list_steps(s.m);
    if (tile)
        hipLaunchKernelGGL(morph_mask_kernel<true>, grid, block, 0, stream, s, c, op, steps, masks, part);
    else
        hipLaunchKernelGGL(morph_mask_kernel<false>, grid, block, 0, stream, s, c, op, steps, masks, part);
    return hipGetLastError();
}

hipError_t launch_morph_keep(const MorphSet& s, uint32_t c, const uint32_t* masks, const uint64_t* part, uint64_t* out_keys,
                             uint32_t* out_words, hipStream_t stream) {
    hipLaunchKernelGGL(morph_keep_kernel, dim3(morph_blocks(s.m)), dim3(kMorphThreads), 0, stream, s, c, masks, part, out_keys, out_words);
    return hipGetLastError();
}

hipError_t launch_morph_offer(const MorphSet& s, uint32_t c, const uint32_t* masks, const uint64_t* part, uint64_t* out_offers,
                              uint32_t* out_words, hipStream_t stream) {
    hipLaunchKernelGGL(morph_offer_kernel, dim3(morph_blocks(s.m)), dim3(kMorphThreads), 0, stream, s, c, masks, part, out_offers, out_words);
    return hipGetLastError();
}

}  // namespace vxrt
