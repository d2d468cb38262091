// query.hip — device side of vxrt_query.h: the voxel lookup (query_lookup_kernel) and the pick (query_pick_kernel, vxrt_edit.h's
// vxrt_pick included) on the 8-byte records (kernels.h: SvoRecord).  The host side is api_query.hip, and api_edit.hip for vxrt_pick;
// the kernels' contract is in query.h and the argument in DESIGN.md §22.
//
// A node's slot s (s = x << 2 | y << 1 | z) holds, as in the walk (trace_common.h: walk_step) and the extract (extract.hip), child
// record / leaf word  base + popc(mask & (bit(s) - 1)).  Following those pointers from the root reads the tree in any layout the
// records can have: the breadth-first build, the holes and 8-entry blocks edits leave (edit.hip), the compacted records, the
// depth-first treelets of VXRT_OPT_NODE_ORDER 2 / 3.
//
// Unique result: every word written is a function of the scene and the entry alone; the count is an integer sum.  Bounds: the
// lookup's loops are over fixed counts (kQueryItems entries, at most kQueryLevels levels); the pick's walk is the tracers', with its
// 2048-trip cap.  No workgroup waits for another.
#include "trace_common.h"
#include "block_scan.h"
#include "query.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kQueryThreads / 64;

// bit k of (x, y, z) as a slot; xy = x << 16 | y
__device__ __forceinline__ uint32_t slot_at(uint32_t xy, uint32_t z, uint32_t k) {
    return ((xy >> (16u + k)) & 1u) << 2 | ((xy >> k) & 1u) << 1 | ((z >> k) & 1u);
}

// One descent per entry, kQueryItems entries per thread.  The entries of a thread go down the tree level by level TOGETHER: the
// loads of one level — one per entry, independent of each other — are all issued before the first is waited for, so a lane has up
// to kQueryItems descents in flight where a loop over the entries would have one chain of depth + 1 dependent loads after another.
// For that no load may sit behind a branch (the compiler waits for a load before it leaves the load's block): every load is
// unconditional, from a safe index where there is nothing to read — entry n - 1 for a round past the list, record 0 / leaf word 0
// for an entry that is outside the root cube or has met a clear bit — and the value is dropped by a select.  Such an entry carries
// masks == 0 from there on.  The host launches this only for a scene that has record 0 and leaf word 0, and for n > 0.
__global__ __launch_bounds__(kQueryThreads) void query_lookup_kernel(const LookupArgs a) {
    const uint64_t first = uint64_t(blockIdx.x) * kQuerySpan + threadIdx.x;
    const uint32_t d = a.depth;
    const int64_t half = int64_t(1) << d;
    int32_t px[kQueryItems], py[kQueryItems], pz[kQueryItems];
#pragma unroll
    for (uint32_t j = 0; j < kQueryItems; j++) {
        const uint64_t i = first + j * kQueryThreads;
        const int16_t* p = a.pos + 3 * (i < a.n ? i : uint64_t(a.n - 1u));
        px[j] = p[0]; py[j] = p[1]; pz[j] = p[2];
    }
    uint32_t masks[kQueryItems], base[kQueryItems], xy[kQueryItems], z[kQueryItems];
#pragma unroll
    for (uint32_t j = 0; j < kQueryItems; j++) {
        const uint64_t i = first + j * kQueryThreads;
        // u = pos + offset + 2^d in 64 bits: nothing wraps.  Inside the cube every u is below 2^(d + 1), a power of two, so the
        // three tests are one on their union (a negative u has its high bits set).
        const int64_t ux = int64_t(px[j]) + int64_t(a.offset[0]) + half, uy = int64_t(py[j]) + int64_t(a.offset[1]) + half,
                      uz = int64_t(pz[j]) + int64_t(a.offset[2]) + half;
        const bool in = i < a.n && uint64_t(ux | uy | uz) < uint64_t(2 * half);
        masks[j] = in ? a.root_rec.masks : 0u;
        base[j] = a.root_rec.base;
        xy[j] = uint32_t(ux) << 16 | (uint32_t(uy) & 0xffffu);
        z[j] = uint32_t(uz);
    }
    // node levels 0 .. d - 1: the child records
#pragma unroll 1
    for (uint32_t l = 0; l < kQueryLevels - 1u; l++) {
        if (l >= d) break;
        const uint32_t k = d - l;
        uint2 r[kQueryItems];
        bool on[kQueryItems];
#pragma unroll
        for (uint32_t j = 0; j < kQueryItems; j++) {
            const uint32_t bit = 1u << slot_at(xy[j], z[j], k), mask = masks[j] & 0xffu;
            on[j] = (mask & bit) != 0u;
            const uint32_t at = on[j] ? base[j] + uint32_t(__popc(mask & (bit - 1u))) : 0u;
            r[j] = *reinterpret_cast<const uint2*>(a.svo + at);
        }
        __builtin_amdgcn_sched_barrier(0);   // the scheduler otherwise moves the first selects, and their waits, up among the loads
#pragma unroll
        for (uint32_t j = 0; j < kQueryItems; j++) {
            masks[j] = on[j] ? r[j].x : 0u;
            base[j] = r[j].y;
        }
    }
    // node level d: the leaf words
    uint32_t word[kQueryItems];
#pragma unroll
    for (uint32_t j = 0; j < kQueryItems; j++) {
        const uint32_t bit = 1u << slot_at(xy[j], z[j], 0u), mask = (masks[j] >> 8) & 0xffu;
        const bool on = (mask & bit) != 0u;
        const uint32_t w = uint32_t(a.leaves[on ? base[j] + uint32_t(__popc(mask & (bit - 1u))) : 0u]);
        word[j] = on ? w : 0u;
    }
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t j = 0; j < kQueryItems; j++) {
        const uint64_t i = first + j * kQueryThreads;
        if (a.leaf != nullptr && i < a.n) a.leaf[i] = word[j];
        mine += word[j] != 0u ? 1u : 0u;
    }
    if (a.part == nullptr) return;   // uniform over the grid
    block_sum_to<kWaves>(mine, a.part + blockIdx.x);
}

// vxrt_pick (max_time == nullptr: every ray unbounded) and vxrt_pick_device: cast_ray (trace_common.h) with its max_distance per ray —
// the same two walks, chosen by cast_ray's own test (the walk with the plane times in registers for a regular, unbounded ray, the
// shader's text otherwise) — and, for a hit, the voxel from the walk's integer path coordinates: at the leaf parent (level lvl =
// depth) the voxel's index along x is  ix << 1 | octant bit x,  d + 1 bits, and its vxrt_set_voxels coordinate is that minus 2^depth
// (scene_host.cpp: build_octree's slot rule).
__global__ __launch_bounds__(kBlock) void query_pick_kernel(const TraceArgs a, const float* origins, const float* dirs, const float* max_time,
                                                            vxrt_pick_hit* out, unsigned n) {
    extern __shared__ uint2 query_stack[];
    const unsigned i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const SceneView sc = make_scene(a);
    const uint32_t depth = uint32_t(a.node_levels - 1);
    uint2* stack = query_stack + threadIdx.x;
    const f3 o = ld3(origins + 3 * size_t(i)), d = ld3(dirs + 3 * size_t(i));
    const float max_distance = max_time != nullptr ? max_time[i] : kAlmostInfinity;
    const f3 inv = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);
    int status = kWalkMiss;
    f3 center = splat3(0.0f);
    float time = 0.0f;
    uint32_t lvl = 0, octant = 0, leaf = 0, ix = 0, iy = 0, iz = 0;
    bool entered;
    if (ray_is_regular(inv) && max_distance == kAlmostInfinity) {
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
            do { status = walk_step(w, sc, max_distance, stack); } while (status == kWalkOn);
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

hipError_t launch_query_lookup(const LookupArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(query_lookup_kernel, dim3(query_blocks(a.n)), dim3(kQueryThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_query_pick(const TraceArgs& a, const float* origins, const float* dirs, const float* max_time, vxrt_pick_hit* out, unsigned n,
                             hipStream_t s) {
    const size_t lds = size_t(a.stack_levels) * kBlock * sizeof(uint2);
    hipLaunchKernelGGL(query_pick_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), lds, s, a, origins, dirs, max_time, out, n);
    return hipGetLastError();
}

}  // namespace vxrt
