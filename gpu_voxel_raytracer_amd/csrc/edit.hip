// edit.hip — device side of vxrt_edit.h: the in-place scene edit (edit_kernel) and the pick query (pick_kernel) on the 8-byte
// records (kernels.h: SvoRecord).  The host side, which sorts a batch into the segments this kernel walks, is api_edit.hip.
//
// The walk (trace_common.h: walk_step) finds slot s of a node at  base + popc(mask & (bit(s) - 1))  — for child records and leaf
// words alike.  A node's block of children only has to be contiguous; where it lies does not matter.  So an edit:
//   * grows a node by giving it a new block of 8 entries after the end of the array (copying the old entries to their new slots),
//     or, when its block already is such an 8-entry block (base >= the count the build produced), by widening it in place;
//   * shrinks a node by compacting its block in place (the block keeps its capacity: a tight block of the build stays "tight",
//     so a node in one moves at most once, to an 8-entry block, and never again);
//   * prunes every node whose masks drop to 0 from its parent, up to the root, so that every mask is what a fresh build has.
// Allocation is by block-wide prefix sums in segment order: the same scene and the same batch give the same records, bit for bit.
#include "trace_common.h"
#include "edit.h"

namespace vxrt {
namespace {

constexpr int kEditThreads = 1024;
constexpr uint32_t kNone = 0xffffffffu;

// exclusive prefix sum of `v` over the block; *total = the sum of all.  Ends with a barrier (LDS may be reused).
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t* total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int off = 1; off < kEditThreads; off <<= 1) {   // Hillis-Steele: 10 steps for 1024 threads
        const uint32_t add = t >= off ? lds[t - off] : 0u;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const uint32_t incl = lds[t];
    *total = lds[kEditThreads - 1];
    __syncthreads();
    return incl - v;
}

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
    __shared__ uint32_t lds[kEditThreads];
    __shared__ uint32_t wave_sum[kEditThreads / 64];
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
                const uint32_t rank = block_scan(alloc ? 1u : 0u, lds, &total);
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
    // live-record counters: per-wave sums (in wave order), then one lane adds them in order
    uint32_t mine = a.clear ? removed : added;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((t & 63u) == 0u) wave_sum[t >> 6] = mine;
    __syncthreads();
    if (t == 0) {
        uint32_t sum = 0;
        for (int w = 0; w < kEditThreads / 64; w++) sum += wave_sum[w];
        a.out[2] = sum;
        a.out[3] = uint32_t(a.svo[0].masks);
        a.out[4] = a.svo[0].base;
    }
}

// vxrt_pick: cast_ray (trace_common.h) — the same two walks, chosen by the same test — and, for a hit, the voxel from the walk's
// integer path coordinates: at the leaf parent (level lvl = depth) the voxel's index along x is  ix << 1 | octant bit x,  d + 1 bits,
// and its vxrt_set_voxels coordinate is that minus 2^depth (scene_host.cpp: build_octree's slot rule).
__global__ __launch_bounds__(kBlock) void pick_kernel(const TraceArgs a, const float* origins, const float* dirs, vxrt_pick_hit* out, unsigned n) {
    extern __shared__ uint2 pick_stack[];
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const SceneView sc = make_scene(a);
    const uint32_t depth = uint32_t(a.node_levels - 1);
    uint2* stack = pick_stack + threadIdx.x;
    const f3 o = ld3(origins + 3 * size_t(i)), d = ld3(dirs + 3 * size_t(i));
    const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    int status = kWalkMiss;
    f3 center = splat3(0.0f);
    float time = 0.0f;
    uint32_t lvl = 0, octant = 0, leaf = 0, ix = 0, iy = 0, iz = 0;
    bool entered;
    if (ray_is_regular(inv)) {
        WalkF w;
        entered = walkf_begin(w, sc, o, d, inv);
        if (entered) {
            do { status = walkf_step(w, sc, stack); } while (status == kWalkOn);
            const uint32_t bit = 1u << w.octant;
            center = w.center; time = w.time; lvl = w.lvl; octant = w.octant;
            ix = w.ix; iy = w.iy; iz = w.iz;
            leaf = w.rec.base + __popc((w.rec.masks >> 8) & (bit - 1u));
        }
    } else {
        Walk w;
        entered = walk_begin(w, sc, o, d);
        if (entered) {
            do { status = walk_step(w, sc, kAlmostInfinity, stack); } while (status == kWalkOn);
            center = w.center; time = w.time; lvl = w.lvl; octant = w.octant;
            ix = w.ix; iy = w.iy; iz = w.iz;
            leaf = walk_leaf_index(w);
        }
    }
    RayHit hit;
    hit.time = 0.0f; hit.node = 0; hit.normal = splat3(0.0f);
    vxrt_pick_hit r{};
    if (entered && finish_ray(sc, status, o, d, time, center, lvl, octant, leaf, hit)) {
        r.status = status == kWalkCap ? 2u : 1u;
        if (status == kWalkLeaf) {
            const int32_t half = int32_t(1) << depth;
            r.voxel[0] = int32_t(ix << 1 | ((octant >> 2) & 1u)) - half;
            r.voxel[1] = int32_t(iy << 1 | ((octant >> 1) & 1u)) - half;
            r.voxel[2] = int32_t(iz << 1 | (octant & 1u)) - half;
        }
    }
    r.time = hit.time;
    r.normal[0] = hit.normal.x; r.normal[1] = hit.normal.y; r.normal[2] = hit.normal.z;
    r.leaf = hit.node;
    out[i] = r;
}

}  // namespace

hipError_t launch_edit(const EditArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(edit_kernel, dim3(1), dim3(kEditThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_pick(const TraceArgs& a, const float* origins, const float* dirs, vxrt_pick_hit* out, unsigned n, hipStream_t s) {
    const size_t lds = size_t(a.stack_levels) * kBlock * sizeof(uint2);
    hipLaunchKernelGGL(pick_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), lds, s, a, origins, dirs, out, n);
    return hipGetLastError();
}

}  // namespace vxrt
