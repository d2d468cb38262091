// pieces.hip — device side of vxrt_pieces.h: per component of a labelled voxel list its size, bounding box, coordinate sums and
// number.  The host side, which runs the labelling (components.h: label_list) and then these launches, is api_pieces.hip; the
// kernels' contract is in pieces.h and the argument in DESIGN.md §21.
//
//   slots     per root its rank among the roots (the flatten's per-block root counts, scanned, plus a block prefix sum) and the
//             start values of its accumulators
//   reduce    over the unique voxels in key order, where a component forms long runs: each run of equal roots is reduced inside its
//             wave (a plain wave reduction where the wave is one run, a segmented scan otherwise) and only the run's last lane adds
//             to the component's accumulators
//   mark      per component: selected or not, and a mark at its label in an array over the input indices
//   number    count / scan of the marks (components_select_count, launch_exclusive_scan), then per mark the component's number
//   emit      per component its vxrt_piece
//   scatter   the list call: label and id per sorted entry, written at the entry's input index
//   pick / write   the scene call: the selected voxels flagged in path order, and each returned voxel's piece number
//
// Unique result: the atomics are integer adds, minima and maxima into a component's accumulators, whose values do not depend on the
// order of arrival; every offset and every number is a prefix sum in entry order.  Bounds: every loop runs over a fixed count
// (kCompItems rounds, 6 scan steps, 16 key levels).  No workgroup waits for another, and the number of launches depends on n only.
#include "block_scan.h"
#include "pieces.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kCompThreads / 64;

// Unique result: a root's slot is the scanned part[block] plus a block prefix sum in entry order; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void pieces_slots_kernel(const uint32_t* comp, const uint32_t* acc, uint32_t m, const uint64_t* part,
                                                                    uint32_t anchored, uint32_t* slot, PieceAcc* accs) {
    __shared__ uint32_t lds[kWaves];
    uint64_t at = part[blockIdx.x];   // the roots before this block
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        const bool root = i < m && comp[i] == uint32_t(i);
        uint32_t total;
        const uint64_t c = at + block_exclusive<uint32_t, kWaves>(root ? 1u : 0u, lds, &total);
        at += total;
        if (!root) continue;
        slot[i] = uint32_t(c);
        PieceAcc* a = accs + c;
        a->count = 0u;
        a->first = kCompNone;
        a->start = 0u;
        a->id = anchored != 0u && acc[i] == 0u ? kPieceHeld : kCompNone;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            a->sum[ax] = 0ull;
            a->lo[ax] = 0xffffffffu;
            a->hi[ax] = 0u;
        }
    }
}

// what a lane, a run or a wave contributes to a component: 11 words; a wave's sums fit 32 bits (64 x 65535)
struct Part {
    uint32_t count, first, lo[3], hi[3], sum[3];
};

__device__ __forceinline__ void add_to(PieceAcc* a, const Part& p) {
    atomicAdd(&a->count, p.count);
    atomicMin(&a->first, p.first);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        atomicMin(&a->lo[ax], p.lo[ax]);
        atomicMax(&a->hi[ax], p.hi[ax]);
        atomicAdd(&a->sum[ax], (unsigned long long)p.sum[ax]);
    }
}

__device__ __forceinline__ void merge(Part& p, const Part& q) {
    p.count += q.count;
    p.first = min(p.first, q.first);
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        p.lo[ax] = min(p.lo[ax], q.lo[ax]);
        p.hi[ax] = max(p.hi[ax], q.hi[ax]);
        p.sum[ax] += q.sum[ax];
    }
}

// A launch after the slots, so accs[] holds its start values.  In a wave's 64 consecutive unique voxels the runs of equal roots are
// cut at the lanes whose root differs from the lane before (lane 0 always; the lanes past m carry kCompNone, which is no root, and
// form a run of their own that adds nothing).  A round whose 64 voxels are one run is not added at once: the wave carries it to its
// next such round and merges the two where the root is the same (8 x 64 x 65535 still fits 32 bits), so a block inside one large
// component adds once per wave.  Atomics: 11 per run and wave otherwise, whatever the run's length.  Unique result: see the head of
// the file.  Bounds: kCompItems rounds, 6 scan steps.
__global__ __launch_bounds__(kCompThreads) void pieces_reduce_kernel(const uint64_t* ukeys, const uint32_t* uhead, const uint32_t* comp,
                                                                     const uint32_t* slot, uint32_t m, PieceAcc* accs) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t carried = kCompNone;   // the root of the whole-wave runs carried so far (the same in every lane), or none
    Part carry = {};
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i - lane >= m) break;   // the whole wave lies past the list; later rounds lie further on
        const bool ok = i < m;
        const uint32_t r = ok ? comp[i] : kCompNone;
        Part p;
        p.count = ok ? 1u : 0u;
        p.first = ok ? uhead[i] : kCompNone;
        uint32_t u[3] = {0u, 0u, 0u};
        if (ok) cell_of(ukeys[i], u);
#pragma unroll
        for (int ax = 0; ax < 3; ax++) p.lo[ax] = p.hi[ax] = p.sum[ax] = u[ax];
        const uint32_t before = __shfl_up(r, 1, 64);
        const bool head = lane == 0u || before != r;
        const uint64_t heads = __ballot(head);
        if (heads == 1ull) {   // one run (lane 0 is valid, so every lane is): a plain wave reduction
            p.count = 64u;
            p.first = wave_min(p.first);
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                p.lo[ax] = wave_min(p.lo[ax]);
                p.hi[ax] = wave_max(p.hi[ax]);
                p.sum[ax] = wave_sum(p.sum[ax]);
            }
            if (carried == r) {
                merge(carry, p);
            } else {
                if (carried != kCompNone && lane == 0u) add_to(accs + slot[carried], carry);
                carried = r;
                carry = p;
            }
            continue;
        }
        // an inclusive scan that stops at the run's first lane: the highest head at or below this lane
        const uint32_t start = 63u - uint32_t(__builtin_clzll(heads & ((2ull << lane) - 1ull)));
#pragma unroll
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            Part q;
            q.count = __shfl_up(p.count, off, 64);
            q.first = __shfl_up(p.first, off, 64);
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                q.lo[ax] = __shfl_up(p.lo[ax], off, 64);
                q.hi[ax] = __shfl_up(p.hi[ax], off, 64);
                q.sum[ax] = __shfl_up(p.sum[ax], off, 64);
            }
            if (lane >= start + off) merge(p, q);
        }
        const bool last = lane == 63u || ((heads >> (lane + 1u)) & 1ull) != 0ull;
        if (ok && last) add_to(accs + slot[r], p);
    }
    if (carried != kCompNone && lane == 0u) add_to(accs + slot[carried], carry);
}

// A launch after the reduce, so the accumulators are final.  Unique result: the labels of two components differ, so every word of
// mark is written at most once; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void pieces_mark_kernel(PieceAcc* accs, uint32_t k, uint32_t n, uint32_t min_voxels,
                                                                   uint32_t max_voxels, uint32_t* mark) {
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t c = entry_of(j);
        if (c >= k) return;
        PieceAcc* a = accs + c;
        const bool selected = a->id != kPieceHeld && a->count >= min_voxels && a->count <= max_voxels;
        a->id = selected ? 0u : kCompNone;   // a selected one gets its number from pieces_number
        if (selected && a->first < n) mark[a->first] = uint32_t(c) + 1u;   // every component has an entry, so first < n
    }
}

// Unique result: sorted is a permutation of the indices, so every word of pick is written once; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void pieces_pick_kernel(const uint32_t* sorted, const uint32_t* rank, uint32_t n, const uint32_t* comp,
                                                                   const uint32_t* slot, const PieceAcc* accs, uint32_t* pick) {
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i >= n) return;
        const uint32_t c = slot[comp[rank[i]]];
        pick[sorted[i]] = accs[c].id != kCompNone ? c + 1u : 0u;
    }
}

// Unique result: every number is the scanned part[block] plus a block prefix sum in entry order; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void pieces_number_kernel(const uint32_t* mark, uint32_t n, const uint64_t* mark_part, const uint32_t* pick,
                                                                     const uint64_t* pick_part, PieceAcc* accs) {
    __shared__ uint32_t lds[kWaves];
    uint64_t at = mark_part[blockIdx.x], picked = pick ? pick_part[blockIdx.x] : 0ull;
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        const uint32_t c1 = i < n ? mark[i] : 0u;
        uint32_t total;
        const uint64_t id = at + block_exclusive<uint32_t, kWaves>(c1 != 0u ? 1u : 0u, lds, &total);
        at += total;
        uint64_t start = 0;
        if (pick) {   // uniform over the block
            start = picked + block_exclusive<uint32_t, kWaves>(i < n && pick[i] != 0u ? 1u : 0u, lds, &total);
            picked += total;
        }
        if (c1 != 0u) {
            accs[c1 - 1u].id = uint32_t(id);
            accs[c1 - 1u].start = uint32_t(start);
        }
    }
}

// A launch after the numbering.  Unique result: the numbers of two selected components differ; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void pieces_emit_kernel(const PieceAcc* accs, uint32_t k, uint32_t scene, vxrt_piece* info) {
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t c = entry_of(j);
        if (c >= k) return;
        const PieceAcc* a = accs + c;
        if (a->id == kCompNone) continue;
        vxrt_piece* out = info + a->id;
        out->first = scene ? a->start : a->first;
        out->voxels = a->count;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            out->min[ax] = int16_t(int32_t(a->lo[ax]) - 32768);
            out->max[ax] = int16_t(int32_t(a->hi[ax]) - 32768);
            out->sum[ax] = int64_t(a->sum[ax]) - 32768ll * int64_t(a->count);   // the bias leaves in 64 bits
        }
        out->reserved = 0u;
    }
}

// Unique result: sorted is a permutation of the indices, so every word is written once; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void pieces_scatter_kernel(const uint32_t* sorted, const uint32_t* rank, uint32_t n, const uint32_t* comp,
                                                                      const uint32_t* slot, const PieceAcc* accs, uint32_t* label, uint32_t* id) {
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        if (i >= n) return;
        const PieceAcc* a = accs + slot[comp[rank[i]]];
        const uint32_t at = sorted[i];
        if (label) label[at] = a->first;
        if (id) id[at] = a->id;
    }
}

// Unique result: every offset is the scanned part[block] plus a block prefix sum in entry order; no atomic.  Bound: kCompItems rounds.
__global__ __launch_bounds__(kCompThreads) void pieces_write_kernel(const uint32_t* pick, uint32_t n, const uint64_t* pick_part, const PieceAcc* accs,
                                                                    uint32_t* piece) {
    __shared__ uint32_t lds[kWaves];
    uint64_t at = pick_part[blockIdx.x];
#pragma unroll 1
    for (uint32_t j = 0; j < kCompItems; j++) {
        const uint64_t i = entry_of(j);
        const uint32_t c1 = i < n ? pick[i] : 0u;
        uint32_t total;
        const uint64_t o = at + block_exclusive<uint32_t, kWaves>(c1 != 0u ? 1u : 0u, lds, &total);
        at += total;
        if (c1 != 0u) piece[o] = accs[c1 - 1u].id;
    }
}

}  // namespace

hipError_t pieces_slots(const uint32_t* comp, const uint32_t* acc, uint32_t m, const uint64_t* part, uint32_t anchored, uint32_t* slot,
                        PieceAcc* accs, hipStream_t s) {
    hipLaunchKernelGGL(pieces_slots_kernel, dim3(comp_blocks(m)), dim3(kCompThreads), 0, s, comp, acc, m, part, anchored, slot, accs);
    return hipGetLastError();
}

hipError_t pieces_reduce(const uint64_t* ukeys, const uint32_t* uhead, const uint32_t* comp, const uint32_t* slot, uint32_t m, PieceAcc* accs,
                         hipStream_t s) {
    hipLaunchKernelGGL(pieces_reduce_kernel, dim3(comp_blocks(m)), dim3(kCompThreads), 0, s, ukeys, uhead, comp, slot, m, accs);
    return hipGetLastError();
}

hipError_t pieces_mark(PieceAcc* accs, uint32_t k, uint32_t n, uint32_t min_voxels, uint32_t max_voxels, uint32_t* mark, hipStream_t s) {
    hipLaunchKernelGGL(pieces_mark_kernel, dim3(comp_blocks(k)), dim3(kCompThreads), 0, s, accs, k, n, min_voxels, max_voxels, mark);
    return hipGetLastError();
}

hipError_t pieces_pick(const uint32_t* sorted, const uint32_t* rank, uint32_t n, const uint32_t* comp, const uint32_t* slot, const PieceAcc* accs,
                       uint32_t* pick, hipStream_t s) {
    hipLaunchKernelGGL(pieces_pick_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, sorted, rank, n, comp, slot, accs, pick);
    return hipGetLastError();
}

hipError_t pieces_number(const uint32_t* mark, uint32_t n, const uint64_t* mark_part, const uint32_t* pick, const uint64_t* pick_part,
                         PieceAcc* accs, hipStream_t s) {
    hipLaunchKernelGGL(pieces_number_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, mark, n, mark_part, pick, pick_part, accs);
    return hipGetLastError();
}

hipError_t pieces_emit(const PieceAcc* accs, uint32_t k, uint32_t scene, vxrt_piece* info, hipStream_t s) {
    hipLaunchKernelGGL(pieces_emit_kernel, dim3(comp_blocks(k)), dim3(kCompThreads), 0, s, accs, k, scene, info);
    return hipGetLastError();
}

hipError_t pieces_scatter(const uint32_t* sorted, const uint32_t* rank, uint32_t n, const uint32_t* comp, const uint32_t* slot,
                          const PieceAcc* accs, uint32_t* label, uint32_t* id, hipStream_t s) {
    hipLaunchKernelGGL(pieces_scatter_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, sorted, rank, n, comp, slot, accs, label, id);
    return hipGetLastError();
}

hipError_t pieces_write(const uint32_t* pick, uint32_t n, const uint64_t* pick_part, const PieceAcc* accs, uint32_t* piece, hipStream_t s) {
    hipLaunchKernelGGL(pieces_write_kernel, dim3(comp_blocks(n)), dim3(kCompThreads), 0, s, pick, n, pick_part, accs, piece);
    return hipGetLastError();
}

}  // namespace vxrt
