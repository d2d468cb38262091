// transform.hip — device side of vxrt_transform.h: the pull of a destination box through a fixed-point affine map into a sorted
// source list (transform_pull_kernel) and the decode of the sorted result (transform_decode_kernel).  The host side is
// api_transform.hip; the rule's arithmetic is transform_rule.h's, the kernels' contract is in transform.h and the argument in
// DESIGN.md §23.
//
// Unique result: every word written is a function of the list, the map and the cell alone; the counts are integer sums in thread
// order.  Bounds: every loop runs a fixed count (kPullItems cells, at most 10 steps in LDS and 32 in global memory); no workgroup
// waits for another.
#include "block_scan.h"
#include "transform.h"
#include "transform_rule.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kPullThreads / 64;

// -DVXRT_TRANSFORM_NO_SAMPLE (an A/B build, scripts/ab_build.sh): every search step reads global memory — what the staged keys are
// measured against
#ifdef VXRT_TRANSFORM_NO_SAMPLE
constexpr bool kStaged = false;
#else
constexpr bool kStaged = true;
#endif

struct Cell { int32_t d[3]; };

__device__ __forceinline__ Cell cell_of(const PullArgs& a, uint32_t c) {
    const uint32_t yz = a.ext[1] * a.ext[2];      // < 2^32: the box has fewer cells than that
    const uint32_t x = c / yz, r = c - x * yz, y = r / a.ext[2], z = r - y * a.ext[2];
    return Cell{{a.lo[0] + int32_t(x), a.lo[1] + int32_t(y), a.lo[2] + int32_t(z)}};
}

// Can no cell of the block pull a voxel?  The block's cells c0 .. c1 lie in the box [lo, hi] of cells taken below; per source axis the
// pulled P of rule 2 over that box lies between the sums of the terms' least and greatest values, each term being monotonic in its
// coordinate, and so does its floor.  An interval that misses the source's bounding box on one axis fails every cell of the block.
// The test only ever drops cells that the search would drop: it depends on blockIdx alone, so the block decides as one.
__device__ __forceinline__ bool block_misses_source(const PullArgs& a, uint32_t c0, uint32_t c1) {
    const Cell p = cell_of(a, c0), q = cell_of(a, c1);
    int32_t lo[3] = {p.d[0], a.lo[1], a.lo[2]};
    int32_t hi[3] = {q.d[0], a.lo[1] + int32_t(a.ext[1]) - 1, a.lo[2] + int32_t(a.ext[2]) - 1};
    if (p.d[0] == q.d[0]) {
        lo[1] = p.d[1]; hi[1] = q.d[1];
        if (p.d[1] == q.d[1]) { lo[2] = p.d[2]; hi[2] = q.d[2]; }
    }
    bool miss = false;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        int64_t least = 2 * a.t[i], most = 2 * a.t[i];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int64_t u = int64_t(a.m[i][j]) * (2 * int64_t(lo[j]) + 1), v = int64_t(a.m[i][j]) * (2 * int64_t(hi[j]) + 1);
            least += u < v ? u : v;
            most += u < v ? v : u;
        }
        miss = miss || (most >> 17) < int64_t(a.src_lo[i]) || (least >> 17) > int64_t(a.src_hi[i]);
    }
    return miss;
}

// One search per cell, kPullItems cells per thread.  The searches of a thread advance TOGETHER, step by step, as the descents of
// query_lookup_kernel do: the loads of one step — one per cell, independent of each other — are all issued before the first is
// waited for, so a lane has up to kPullItems searches in flight where a loop over the cells would run one chain of log2(count)
// dependent loads after another.  For that no load may sit behind a branch: every load is unconditional.  A cell that failed the
// range test searches for key 0 and a round past the box for the block's last cell — every index a search visits lies in
// [0, count) whatever the key — and a select drops the answer.  (The key of a failed cell is chosen by a branch around the bit
// spreading, not by a select after it: computed for all eight cells at once the spreading costs 44 registers and a wave per SIMD.)
//
// The search keeps the invariant "the last key <= k, if there is one, is in [base, base + len)": one step halves len (to its ceiling),
// and a step at len == 1 reads keys[base] and moves nothing, so a fixed step count serves ranges whose lengths differ by one.
//
// kStaged: the block first stages kPullSample keys in LDS — the whole list when it is that short, else keys[i * count / 1024] — and
// the first steps read those; the steps in global memory then search only between two neighbouring samples.
template <bool kEmit>
__global__ __launch_bounds__(kPullThreads) void transform_pull_kernel(const PullArgs a) {
    __shared__ uint64_t sample[kStaged ? kPullSample : 1];
    const uint32_t c0 = blockIdx.x * kPullSpan;
    const uint32_t c1 = a.cells - c0 > kPullSpan ? c0 + kPullSpan - 1u : a.cells - 1u;
    if (block_misses_source(a, c0, c1)) {
        if (!kEmit && threadIdx.x == 0) a.part[blockIdx.x] = 0;
        return;
    }
    const bool sampled = kStaged && a.count > kPullSample;
    if (kStaged) {
        uint64_t staged[kPullSample / kPullThreads];
#pragma unroll
        for (uint32_t k = 0; k < kPullSample / kPullThreads; k++) {
            const uint32_t i = k * kPullThreads + threadIdx.x;
            staged[k] = a.keys[sampled ? uint32_t((uint64_t(i) * a.count) >> 10) : min(i, a.count - 1u)];
        }
#pragma unroll
        for (uint32_t k = 0; k < kPullSample / kPullThreads; k++) sample[k * kPullThreads + threadIdx.x] = staged[k];
        __syncthreads();
    }

    uint64_t key[kPullItems];
    bool ok[kPullItems];
#pragma unroll
    for (uint32_t j = 0; j < kPullItems; j++) {
        const uint32_t c = c0 + j * kPullThreads + threadIdx.x;
        const bool live = c <= c1;
        const Cell cell = cell_of(a, live ? c : c1);
        int64_t s[3];
        pull_cell(a.m, a.t, cell.d, s);
        ok[j] = live && pull_in_range(s);
        key[j] = ok[j] ? path_key15(int32_t(s[0]), int32_t(s[1]), int32_t(s[2])) : 0u;
    }

    uint32_t base[kPullItems], len[kPullItems];
#pragma unroll
    for (uint32_t j = 0; j < kPullItems; j++) { base[j] = 0u; len[j] = kStaged ? 1u : a.count; }
    if (kStaged) {
        // the staged keys: a.count of them, or kPullSample
#pragma unroll 1
        for (uint32_t n = sampled ? kPullSample : a.count; n > 1u; n -= n >> 1) {
            const uint32_t half = n >> 1;
#pragma unroll
            for (uint32_t j = 0; j < kPullItems; j++) base[j] = sample[base[j] + half] <= key[j] ? base[j] + half : base[j];
        }
        if (sampled) {
#pragma unroll
            for (uint32_t j = 0; j < kPullItems; j++) {
                const uint32_t from = uint32_t((uint64_t(base[j]) * a.count) >> 10), to = uint32_t((uint64_t(base[j] + 1u) * a.count) >> 10);
                base[j] = from;
                len[j] = to - from;     // >= 1: count > kPullSample
            }
        }
    }
#pragma unroll 1
    for (uint32_t step = 0; step < a.steps; step++) {
        uint64_t v[kPullItems];
        uint32_t half[kPullItems];
#pragma unroll
        for (uint32_t j = 0; j < kPullItems; j++) {
            half[j] = len[j] >> 1;
            v[j] = a.keys[base[j] + half[j]];
        }
        __builtin_amdgcn_sched_barrier(0);   // the scheduler otherwise moves the first selects, and their waits, up among the loads
#pragma unroll
        for (uint32_t j = 0; j < kPullItems; j++) {
            base[j] = v[j] <= key[j] ? base[j] + half[j] : base[j];
            len[j] -= half[j];
        }
    }
    uint64_t at[kPullItems];
    uint32_t word[kPullItems];
#pragma unroll
    for (uint32_t j = 0; j < kPullItems; j++) {
        at[j] = a.keys[base[j]];
        word[j] = kEmit && a.words != nullptr ? uint32_t(a.words[base[j]]) : 0u;
    }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kPullItems; j++) {
        ok[j] = ok[j] && at[j] == key[j];
        mine += ok[j] ? 1u : 0u;
    }
    if (!kEmit) {
        block_sum_to<kWaves>(mine, a.part + blockIdx.x);
        return;
    }
    __shared__ uint32_t scan[kWaves];
    uint32_t total;
    uint64_t to = a.part[blockIdx.x] + block_exclusive<uint32_t, kWaves>(mine, scan, &total);
#pragma unroll
    for (uint32_t j = 0; j < kPullItems; j++) {
        if (ok[j]) {
            const Cell cell = cell_of(a, c0 + j * kPullThreads + threadIdx.x);
            a.out_keys[to] = path_key15(cell.d[0], cell.d[1], cell.d[2]);
            if (a.out_words != nullptr) a.out_words[to] = word[j];
            to++;
        }
    }
}

// bits 3k of v, k = 0 .. 15 -> a coordinate of the int16 range
__device__ __forceinline__ int32_t gather16(uint64_t v) {
    uint32_t u = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; k++) u |= uint32_t((v >> (3u * k)) & 1u) << k;
    return int32_t(u) - 32768;
}

__global__ __launch_bounds__(kPullThreads) void transform_decode_kernel(const uint64_t* keys, const uint32_t* words, uint32_t n, uint8_t* pos,
                                                                        uint8_t* mrgb) {
    const uint32_t i = blockIdx.x * kPullThreads + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = keys[i];
    const int32_t p[3] = {gather16(k >> 2), gather16(k >> 1), gather16(k)};
    uint8_t* o = pos + 6 * size_t(i);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        o[2 * ax] = uint8_t(uint32_t(p[ax]) & 0xffu);
        o[2 * ax + 1] = uint8_t((uint32_t(p[ax]) >> 8) & 0xffu);
    }
    if (mrgb != nullptr) {
        const uint32_t w = words[i];
        uint8_t* b = mrgb + 4 * size_t(i);
        b[0] = uint8_t((w >> 24) & 0x7fu);
        b[1] = uint8_t((w >> 16) & 0xffu);
        b[2] = uint8_t((w >> 8) & 0xffu);
        b[3] = uint8_t(w & 0xffu);
    }
}

uint32_t ceil_log2(uint32_t v) {
    uint32_t bits = 0;
    while ((uint64_t(1) << bits) < v) bits++;
    return bits;
}

}  // namespace

hipError_t launch_transform_pull(const PullArgs& args, hipStream_t s) {
    PullArgs a = args;
    // the steps in global memory: over the whole list, or between two neighbouring samples (at most ceil(count / kPullSample) keys)
    a.steps = !kStaged ? ceil_log2(a.count) : a.count > kPullSample ? ceil_log2(uint32_t((uint64_t(a.count) + kPullSample - 1) / kPullSample)) : 0u;
    const dim3 grid(pull_blocks(a.cells)), block(kPullThreads);
    if (a.out_keys != nullptr)
        hipLaunchKernelGGL(transform_pull_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(transform_pull_kernel<false>, grid, block, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_transform_decode(const uint64_t* keys, const uint32_t* words, uint32_t n, uint8_t* pos, uint8_t* mrgb, hipStream_t s) {
    hipLaunchKernelGGL(transform_decode_kernel, dim3((n + kPullThreads - 1) / kPullThreads), dim3(kPullThreads), 0, s, keys, words, n, pos, mrgb);
    return hipGetLastError();
}

}  // namespace vxrt
