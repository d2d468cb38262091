// edit.hip — device side of vxrt_edit.h: the in-place scene edit (edit_kernel) on the 8-byte records (kernels.h: SvoRecord).  The
// host side, which sorts a batch into the segments this kernel walks, is api_edit.hip; vxrt_pick's kernel is query.hip's.
//
// The walk (trace_common.h: walk_step) finds slot s of a node at  base + popc(mask & (bit(s) - 1))  — for child records and leaf
// words alike.  A node's block of children only has to be contiguous; where it lies does not matter.  So an edit:
//   * grows a node by giving it a new block of 8 entries after the end of the array (copying the old entries to their new slots),
//     or, when its block already is such an 8-entry block (base >= the count the build produced), by widening it in place;
//   * shrinks a node by compacting its block in place (the block keeps its capacity: a tight block of the build stays "tight",
//     so a node in one moves at most once, to an 8-entry block, and never again);
//   * prunes every node whose masks drop to 0 from its parent, up to the root, so that every mask is what a fresh build has.
// Allocation is by block-wide prefix sums in segment order: the same scene and the same batch give the same records, bit for bit.
#include "block_scan.h"
#include "edit.h"

namespace vxrt {
namespace {

constexpr int kEditThreads = 1024;
constexpr uint32_t kEditWaves = kEditThreads / 64;
constexpr uint32_t kNone = 0xffffffffu;

// stores of this thread reach the CU's memory before the barrier that follows (the next level reads them from other waves)
__device__ __forceinline__ void level_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

__device__ __forceinline__ uint32_t need_mask(const EditArgs& a, uint32_t s) {
    uint32_t m = 0;
    for (uint32_t c = a.child_begin[s]; c < a.child_begin[s + 1]; c++) m |= 1u << a.oct[c];
    return m;
}

__device__ __forceinline__ uint32_t slot_index(uint32_t base, uint32_t mask, uint32_t slot) {
    return base + uint32_t(__popc(mask & ((1u << slot) - 1u)));
}

// One workgroup: the levels of a batch depend on each other, and a batch is small next to the work of one workgroup (a few loads
// per touched node); the levels are separated by barriers, so a batch is one launch.
__global__ __launch_bounds__(kEditThreads) void edit_kernel(const EditArgs a) {
    __shared__ uint32_t lds[kEditWaves];
    const uint32_t t = threadIdx.x;
    const uint32_t L = a.depth;   // node levels 0 (root) .. L (leaf parents); segments of level L + 1 are the batch's entries
    uint32_t added = 0, removed = 0;
    if (t == 0) a.node[0] = 0u;   // the root segment is record 0
    level_barrier();

    if (!a.clear) {
        uint32_t svo_top = a.svo_end, leaf_top = a.leaf_end;
        for (uint32_t l = 0; l <= L; l++) {
            const bool leaf_level = l == L;
            const uint32_t s0 = a.seg_off[l], s1 = a.seg_off[l + 1];
            for (uint32_t chunk = s0; chunk < s1; chunk += kEditThreads) {
                const uint32_t s = chunk + t;
                const bool active = s < s1;
                SvoRecord rec{0u, 0u};
                uint32_t node = 0, old = 0, nw = 0;
                bool alloc = false;
                if (active) {
                    node = a.node[s];
                    rec = a.svo[node];
                    old = leaf_level ? (rec.masks >> 8) & 0xffu : rec.masks & 0xffu;
                    nw = old | need_mask(a, s);
                    const bool eight = rec.base >= (leaf_level ? a.leaf_built : a.svo_built);   // an 8-entry block of an earlier edit
                    alloc = nw != old && (old == 0u || !eight);
                }
                uint32_t total;
                const uint32_t rank = block_exclusive<uint32_t, kEditWaves>(alloc ? 1u : 0u, lds, &total);
                if (active) {
                    if (nw != old) {
                        const uint32_t base = alloc ? (leaf_level ? leaf_top : svo_top) + 8u * rank : rec.base;
                        // old entries to their new slots: from the highest slot down, so that widening in place (new index >= old
                        // index) never overwrites an entry before it is moved
                        for (int sl = 7; sl >= 0; sl--) {
                            const uint32_t b = 1u << sl;
                            if (nw & b) {
                                const uint32_t dst = slot_index(base, nw, uint32_t(sl));
                                if (old & b) {
                                    const uint32_t src = slot_index(rec.base, old, uint32_t(sl));
                                    if (leaf_level) a.leaves[dst] = a.leaves[src];
                                    else a.svo[dst] = a.svo[src];
                                } else if (!leaf_level) {
                                    a.svo[dst] = SvoRecord{0u, 0u};   // a new child: filled by the next level
                                }
                            }
                        }
                        if (!leaf_level) added += uint32_t(__popc(nw ^ old));
                        rec.base = base;
                        rec.masks = leaf_level ? (nw << 8) : nw;
                        a.svo[node] = rec;
                    }
                    for (uint32_t c = a.child_begin[s]; c < a.child_begin[s + 1]; c++) {
                        const uint32_t dst = slot_index(rec.base, nw, a.oct[c]);
                        if (leaf_level) a.leaves[dst] = a.words[c - a.seg_off[L + 1]];
                        else a.node[c] = dst;
                    }
                }
                if (leaf_level) leaf_top += 8u * total;
                else svo_top += 8u * total;
            }
            level_barrier();
        }
        if (t == 0) { a.out[0] = svo_top; a.out[1] = leaf_top; }
    } else {
        // top-down: the record of every segment's node, or kNone when the path leaves the tree (nothing to clear below)
        for (uint32_t l = 0; l < L; l++) {
            for (uint32_t s = a.seg_off[l] + t; s < a.seg_off[l + 1]; s += kEditThreads) {
                const uint32_t node = a.node[s];
                const SvoRecord rec = node == kNone ? SvoRecord{0u, 0u} : a.svo[node];
                const uint32_t cm = rec.masks & 0xffu;
                for (uint32_t c = a.child_begin[s]; c < a.child_begin[s + 1]; c++)
                    a.node[c] = (cm >> a.oct[c] & 1u) ? slot_index(rec.base, cm, a.oct[c]) : kNone;
            }
            level_barrier();
        }
        // bottom-up: compact every block in place; flag[s] = 1 when segment s's node lost its last entry (its parent drops it)
        for (int l = int(L); l >= 0; l--) {
            const bool leaf_level = uint32_t(l) == L;
            for (uint32_t s = a.seg_off[l] + t; s < a.seg_off[l + 1]; s += kEditThreads) {
                const uint32_t node = a.node[s];
                uint8_t empty = 0;
                if (node != kNone) {
                    SvoRecord rec = a.svo[node];
                    const uint32_t old = leaf_level ? (rec.masks >> 8) & 0xffu : rec.masks & 0xffu;
                    uint32_t rm = 0;
                    for (uint32_t c = a.child_begin[s]; c < a.child_begin[s + 1]; c++)
                        if (leaf_level || a.flag[c]) rm |= 1u << a.oct[c];
                    rm &= old;
                    if (rm) {
                        const uint32_t nw = old & ~rm;
                        uint32_t j = rec.base;
                        for (uint32_t sl = 0; sl < 8; sl++) {   // destination <= source: in place from the lowest slot up
                            if (!(nw >> sl & 1u)) continue;
                            const uint32_t src = slot_index(rec.base, old, sl);
                            if (leaf_level) a.leaves[j] = a.leaves[src];
                            else a.svo[j] = a.svo[src];
                            j++;
                        }
                        for (; j < rec.base + uint32_t(__popc(old)); j++) {   // the freed tail of the block
                            if (leaf_level) a.leaves[j] = 0;
                            else a.svo[j] = SvoRecord{0u, 0u};
                        }
                        if (!leaf_level) removed += uint32_t(__popc(rm));
                        rec.masks = leaf_level ? (nw << 8) : nw;
                        if (nw == 0u && l > 0) rec.base = 0u;   // pruned below: the record itself goes with the parent's compaction
                        a.svo[node] = rec;
                        empty = nw == 0u ? 1 : 0;
                    }
                }
                a.flag[s] = empty;
            }
            level_barrier();
        }
        if (t == 0) { a.out[0] = a.svo_end; a.out[1] = a.leaf_end; }
    }
    block_sum_to<kEditWaves>(a.clear ? removed : added, a.out + 2);   // the live-record counter
    if (t == 0) {
        a.out[3] = uint32_t(a.svo[0].masks);
        a.out[4] = a.svo[0].base;
    }
}

}  // namespace

hipError_t launch_edit(const EditArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(edit_kernel, dim3(1), dim3(kEditThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace vxrt
