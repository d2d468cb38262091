// scene_depth.hip — device side of vxrt_scene_depth.h: levels added on top of a scene's root, or removed from it, in the 8-byte
// records (kernels.h: SvoRecord).  The host side, which decides from the root record and the probe, is api_scene_depth.hip.
//
// Octant o of the root cube [-2^d, 2^d)^3 is the cube of side 2^d at the corner o (x: 4, y: 2, z: 1; a bit set = the upper half).
// One level up it is octant o ^ 7 of the root's octant o: the corner of the larger cube's child that touches the centre.  So a
// level on top turns the root's child o into a node whose only child, in slot o ^ 7, is the old child; a level off the top is
// possible exactly when every child o of the root has slot o ^ 7 only, and replaces it by that grandchild.
//
// Every node a grow makes gets an 8-entry block of its own at the end of the records (or leaf words): edit_kernel widens a block
// at or above the build counts in place (edit.hip), so two nodes must never share one.  A shrink writes only into the root's own
// block; the blocks it unlinks become holes, as the blocks of nodes an edit moves do.
#include "edit.h"

namespace vxrt {
namespace {

constexpr int kDepthThreads = 64;   // one wave; lane o < 8 takes the root's octant o

__device__ __forceinline__ uint32_t child_mask(SvoRecord r, bool leaf_parent) { return leaf_parent ? (r.masks >> 8) & 0xffu : r.masks & 0xffu; }

__device__ __forceinline__ uint32_t rank_in(uint32_t mask, uint32_t o) { return uint32_t(__popc(mask & ((1u << o) - 1u))); }

__global__ __launch_bounds__(kDepthThreads) void depth_probe_kernel(const SvoRecord* svo, SvoRecord root, uint32_t depth, uint32_t* out) {
    const uint32_t o = threadIdx.x;
    const uint32_t M = child_mask(root, depth == 0u);
    uint32_t len = depth;   // a lane without a child does not limit the shrink
    bool single = false;    // lane 0: below its chain of slot 7, the path takes slot 0 only (the voxel (-2^t)^3)
    if (o < 8u && (M >> o & 1u)) {
        uint32_t idx = root.base + rank_in(M, o);
        bool chain = true;
        single = o == 0u;
        len = 0;
        for (uint32_t l = 1; l <= depth && (chain || single); l++) {
            const SvoRecord r = svo[idx];
            const uint32_t m = child_mask(r, l == depth);
            chain = chain && m == (1u << (o ^ 7u));
            if (chain) len++;
            else single = single && m == 1u;
            idx = r.base;   // the only child (the walk ends at a node with more than one)
        }
    }
    for (int off = 32; off > 0; off >>= 1) len = min(len, uint32_t(__shfl_xor(int(len), off)));
    if (o == 0u) {
        out[0] = len;
        out[1] = M == 1u && single ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kDepthThreads) void depth_grow_kernel(SvoRecord* svo, int32_t* leaves, SvoRecord root, uint32_t depth,
                                                                   uint32_t levels, uint32_t svo_end, uint32_t leaf_end) {
    const uint32_t o = threadIdx.x;
    const uint32_t M = child_mask(root, depth == 0u);
    if (o == 0u) svo[0] = SvoRecord{M, svo_end};
    if (o >= 8u || !(M >> o & 1u)) return;
    const uint32_t r = rank_in(M, o), one = 1u << (o ^ 7u);
    const uint32_t blocks = depth == 0u ? levels - 1u : levels;   // record blocks per chain (with depth 0 the last block is leaf words)
    const uint32_t first = svo_end + 8u + 8u * r * blocks;
    uint32_t at = svo_end + r;                                    // the chain's first node: slot r of the root's new block
    for (uint32_t j = 1; j <= levels; j++) {
        if (j == levels && depth == 0u) {
            const uint32_t b = leaf_end + 8u * r;
            leaves[b] = leaves[root.base + r];
            svo[at] = SvoRecord{one << 8, b};
        } else {
            const uint32_t b = first + 8u * (j - 1u);
            if (j == levels) svo[b] = svo[root.base + r];
            svo[at] = SvoRecord{one, b};
            at = b;
        }
    }
}

__global__ __launch_bounds__(kDepthThreads) void depth_shrink_kernel(SvoRecord* svo, int32_t* leaves, SvoRecord root, uint32_t depth,
                                                                     uint32_t levels, uint32_t leaf_end) {
    const uint32_t o = threadIdx.x;
    const uint32_t M = child_mask(root, false);
    if (o == 0u && levels == depth) svo[0] = SvoRecord{M << 8, leaf_end};
    if (o >= 8u || !(M >> o & 1u)) return;
    const uint32_t r = rank_in(M, o), slot = root.base + r;
    uint32_t idx = slot;
    for (uint32_t j = 0; j < levels; j++) idx = svo[idx].base;   // down the path of slot o ^ 7: the record (or leaf word) `levels` below
    if (levels == depth) leaves[leaf_end + r] = leaves[idx];
    else svo[slot] = svo[idx];
}

}  // namespace

hipError_t launch_depth_probe(const SvoRecord* svo, SvoRecord root, uint32_t depth, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(depth_probe_kernel, dim3(1), dim3(kDepthThreads), 0, s, svo, root, depth, out);
    return hipGetLastError();
}

hipError_t launch_depth_grow(SvoRecord* svo, int32_t* leaves, SvoRecord root, uint32_t depth, uint32_t levels, uint32_t svo_end,
                             uint32_t leaf_end, hipStream_t s) {
    hipLaunchKernelGGL(depth_grow_kernel, dim3(1), dim3(kDepthThreads), 0, s, svo, leaves, root, depth, levels, svo_end, leaf_end);
    return hipGetLastError();
}

hipError_t launch_depth_shrink(SvoRecord* svo, int32_t* leaves, SvoRecord root, uint32_t depth, uint32_t levels, uint32_t leaf_end,
                               hipStream_t s) {
    hipLaunchKernelGGL(depth_shrink_kernel, dim3(1), dim3(kDepthThreads), 0, s, svo, leaves, root, depth, levels, leaf_end);
    return hipGetLastError();
}

}  // namespace vxrt
