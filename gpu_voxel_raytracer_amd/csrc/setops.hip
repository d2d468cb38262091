// setops.hip — device side of vxrt_setops.h: the merge of two sorted unique key arrays under a set operation (setop_merge_kernel).
// The host side is api_setops.hip; the co-rank, the membership tests and the keep rule are setops_rule.h's, the kernel's contract is
// in setops.h and the argument in DESIGN.md §24.
//
// Unique result: every word written is a function of the two key arrays, their words and the op alone; the counts are integer sums in
// thread order.  Bounds: every loop runs a fixed count (32 co-rank steps at most, kStageRounds staging loads, kSetopItems items); no
// workgroup waits for another, and there is no atomic.
#include "block_scan.h"
#include "setops.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kSetopThreads / 64;
// the tile: A[a0 - 1 .. a1) and B[b0 .. b1], at most kSetopSpan + 2 keys
constexpr uint32_t kTileKeys = kSetopSpan + 2;
constexpr uint32_t kStageRounds = (kTileKeys + kSetopThreads - 1) / kSetopThreads;

// A block takes the merged items [d0, d1), d0 = kSetopSpan * blockIdx.x.
//  1. Lanes 0 and 1 co-rank the diagonals d0 and d1 in global memory (side by side: the same loop, one wave) and LDS hands the two
//     answers to the block: the tile is A[a0 .. a1) and B[b0 .. b1), b = d - a.
//  2. The block stages A[a0 - 1 .. a1) and, behind it, B[b0 .. b1] — ONE key past the tile's B range, so that an A item whose B
//     cursor stands at the tile's end is tested against the key it could equal without a load of its own; kSetopNoKey stands where
//     the list has no such key.  Element e of the staged run is loaded by thread e % 256 in round e / 256: coalesced, every load
//     unconditional from a clamped index, all of a thread's loads issued before its first wait.
//  3. Each thread co-ranks its diagonal 8 t in LDS and merges its items serially out of LDS (setops_rule.h: merge_run).
// Then the words: the item's own (emitting, or CHANGED) and for CHANGED the word of A[i - 1] — unconditional loads from clamped
// indices, all issued before the first is used, and selects drop what does not apply (no load behind a divergent branch).
template <bool kEmit>
__global__ __launch_bounds__(kSetopThreads) void setop_merge_kernel(const SetopArgs a) {
    __shared__ uint64_t tile[kStageRounds * kSetopThreads];     // kTileKeys are read; the last round's stores need no test of their own
    __shared__ uint32_t ends[2];
    const uint32_t total = a.ma + a.mb;
    const uint32_t d0 = blockIdx.x * kSetopSpan;
    const uint32_t d1 = total - d0 > kSetopSpan ? d0 + kSetopSpan : total;
    if (threadIdx.x < 2u) ends[threadIdx.x] = merge_corank(a.keys_a, a.ma, a.keys_b, a.mb, threadIdx.x ? d1 : d0);
    __syncthreads();
    const uint32_t a0 = ends[0], a1 = ends[1], b0 = d0 - a0, b1 = d1 - a1;
    const uint32_t na = a1 - a0, nb = b1 - b0;

    {
        uint64_t staged[kStageRounds];
#pragma unroll
        for (uint32_t k = 0; k < kStageRounds; k++) {
            const uint32_t e = k * kSetopThreads + threadIdx.x;
            const bool in_a = e <= na;                                  // e = 0 .. na: A[a0 - 1 + e]; then B[b0 + e - na - 1]
            const uint32_t at = in_a ? a0 + e - 1u : b0 + (e - na - 1u);  // wraps where a0 + e == 0: clamped, and dropped below
            staged[k] = (in_a ? a.keys_a : a.keys_b)[safe_index(at, in_a ? a.ma : a.mb)];
        }
#pragma unroll
        for (uint32_t k = 0; k < kStageRounds; k++) {
            const uint32_t e = k * kSetopThreads + threadIdx.x;
            const bool in_a = e <= na;
            const bool there = in_a ? a0 + e != 0u : b0 + (e - na - 1u) < a.mb;    // a0 + e - 1 < a1 <= ma otherwise
            tile[e] = there ? staged[k] : kSetopNoKey;
        }
    }
    __syncthreads();

    const uint32_t items = d1 - d0;
    const uint32_t diag = min(threadIdx.x * kSetopItems, items);
    const uint32_t count = min(kSetopItems, items - diag);
    uint64_t key[kSetopItems];
    uint32_t own[kSetopItems], from_b, matched;
    const uint32_t live = merge_run(tile + 1, na, tile + 1 + na, nb, diag, count, key, own, &from_b, &matched);

    uint32_t word[kSetopItems], other[kSetopItems];
    const bool changed = a.op == kListChanged;
    if (a.words_a != nullptr && (kEmit || changed)) {     // uniform over the grid, and no wait inside
#pragma unroll
        for (uint32_t k = 0; k < kSetopItems; k++) {
            const bool fb = (from_b >> k & 1u) != 0u, of_b = fb && a.words_b != nullptr;     // a mask's items are never kept
            const uint32_t at = (fb ? b0 : a0) + own[k];
            word[k] = (of_b ? a.words_b : a.words_a)[safe_index(at, of_b ? a.mb : a.ma)];
            other[k] = changed ? a.words_a[safe_index(a_index_before(d0 + diag + k, at), a.ma)] : 0u;     // of A[i - 1], for a B item
        }
        __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
        for (uint32_t k = 0; k < kSetopItems; k++) word[k] = other[k] = 0u;
    }
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSetopItems; k++) {
        const bool yes = (live >> k & 1u) != 0u && keep(a.op, (from_b >> k & 1u) != 0u, (matched >> k & 1u) != 0u, word[k] == other[k]);
        kept |= (yes ? 1u : 0u) << k;
    }
    const uint32_t mine = uint32_t(__builtin_popcount(kept));
    if (!kEmit) {
        block_sum_to<kWaves>(mine, a.part + blockIdx.x);
        return;
    }
    __shared__ uint32_t scan[kWaves];
    uint32_t all;
    uint64_t to = a.part[blockIdx.x] + block_exclusive<uint32_t, kWaves>(mine, scan, &all);
#pragma unroll
    for (uint32_t k = 0; k < kSetopItems; k++) {
        if (kept >> k & 1u) {
            a.out_keys[to] = key[k];
            if (a.out_words != nullptr) a.out_words[to] = word[k];
            to++;
        }
    }
}

}  // namespace

hipError_t launch_setop_merge(const SetopArgs& a, hipStream_t s) {
    const dim3 grid(setop_blocks(uint64_t(a.ma) + a.mb)), block(kSetopThreads);
    if (a.out_keys != nullptr)
        hipLaunchKernelGGL(setop_merge_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(setop_merge_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace vxrt
