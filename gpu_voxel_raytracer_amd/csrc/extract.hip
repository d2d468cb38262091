// extract.hip — device side of vxrt_extract.h: the scene's voxels decoded from the 8-byte records (kernels.h: SvoRecord), one node
// level at a time over the whole device.  The host side, which runs the levels and owns the scratch, is api_extract.hip; the scheme
// is in extract.h.
//
// A node's slot s (s = x << 2 | y << 1 | z) holds, as in the walk (trace_common.h: walk_step), child record / leaf word
// base + popc(mask & (bit(s) - 1)).  Following those pointers from the root reads the tree in any layout the records can have: the
// breadth-first build, the holes and 8-entry blocks edits leave (edit.hip), the depth-first treelets of VXRT_OPT_NODE_ORDER 2 / 3.
// Children are visited in ascending slot order and written at prefix offsets, so every frontier, and the output, is in path order.
#include "block_scan.h"
#include "extract.h"

namespace vxrt {
namespace {

// the slots of a node at cell u whose children's cubes meet the box (a.lo, a.hi): per axis, which of the two halves meets it
__device__ __forceinline__ uint32_t box_slots(const ExtractLevel& a, uint32_t ux, uint32_t uy, uint32_t uz) {
    const uint32_t u[3] = {ux, uy, uz};
    uint32_t ok[3];
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        ok[ax] = 0;
#pragma unroll
        for (uint32_t b = 0; b < 2; b++) {
            const uint32_t c = 2u * u[ax] + b;
            if ((c << a.shift) < a.hi[ax] && ((c + 1u) << a.shift) > a.lo[ax]) ok[ax] |= 1u << b;
        }
    }
    uint32_t m = 0;
#pragma unroll
    for (uint32_t s = 0; s < 8; s++) m |= ((ok[0] >> (s >> 2)) & (ok[1] >> ((s >> 1) & 1u)) & (ok[2] >> (s & 1u)) & 1u) << s;
    return m;
}

// the node's slots that exist (child mask, or leaf mask at the leaf parents' level) and meet the box
__device__ __forceinline__ uint32_t kept_slots(const ExtractLevel& a, const uint4 e, SvoRecord* rec) {
    const uint2 r = *reinterpret_cast<const uint2*>(a.svo + e.x);
    rec->masks = r.x;
    rec->base = r.y;
    const uint32_t mask = a.leaf ? (r.x >> 8) & 0xffu : r.x & 0xffu;
    return mask == 0u ? 0u : mask & box_slots(a, e.y, e.z, e.w);
}

__global__ __launch_bounds__(kExtractThreads) void extract_count_kernel(const ExtractLevel a) {
    __shared__ uint32_t lds[kExtractThreads / 64];
    const uint32_t first = blockIdx.x * kExtractSpan + threadIdx.x;
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < kExtractItems; j++) {
        const uint32_t i = first + j * kExtractThreads;
        if (i < a.n) {
            SvoRecord rec;
            sum += uint32_t(__popc(kept_slots(a, a.front[i], &rec)));
        }
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < kExtractThreads / 64; w++) all += lds[w];
        a.part[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kExtractThreads) void extract_expand_kernel(const ExtractLevel a) {
    __shared__ uint32_t lds[kExtractThreads / 64];
    const uint32_t first = blockIdx.x * kExtractSpan + threadIdx.x;
    uint64_t at = a.part[blockIdx.x];   // where this block's first kept child goes
#pragma unroll 1
    for (uint32_t j = 0; j < kExtractItems; j++) {
        const uint32_t i = first + j * kExtractThreads;
        uint4 e = make_uint4(0u, 0u, 0u, 0u);
        SvoRecord rec{0u, 0u};
        uint32_t kept = 0;
        if (i < a.n) {
            e = a.front[i];
            kept = kept_slots(a, e, &rec);
        }
        uint32_t total;
        uint64_t o = at + block_exclusive<uint32_t, kExtractThreads / 64>(uint32_t(__popc(kept)), lds, &total);
        at += total;
        if (kept == 0u) continue;
        const uint32_t mask = a.leaf ? (rec.masks >> 8) & 0xffu : rec.masks & 0xffu;
        for (uint32_t s = 0; s < 8; s++) {
            if (!((kept >> s) & 1u)) continue;
            const uint32_t slot = rec.base + uint32_t(__popc(mask & ((1u << s) - 1u)));
            const uint32_t cx = 2u * e.y + (s >> 2), cy = 2u * e.z + ((s >> 1) & 1u), cz = 2u * e.w + (s & 1u);
            if (a.leaf) {
                const uint32_t w = uint32_t(a.leaves[slot]);
                a.pos[3 * o + 0] = int16_t(int32_t(cx) - int32_t(a.half));
                a.pos[3 * o + 1] = int16_t(int32_t(cy) - int32_t(a.half));
                a.pos[3 * o + 2] = int16_t(int32_t(cz) - int32_t(a.half));
                a.mrgb[o] = __builtin_bswap32(w) & 0xffffff7fu;   // bytes (w >> 24 & 0x7f, w >> 16, w >> 8, w)
            } else {
                a.next[o] = make_uint4(slot, cx, cy, cz);
            }
            o++;
        }
    }
}

}  // namespace

hipError_t launch_extract_count(const ExtractLevel& a, hipStream_t s) {
    hipLaunchKernelGGL(extract_count_kernel, dim3(extract_blocks(a.n)), dim3(kExtractThreads), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_extract_expand(const ExtractLevel& a, hipStream_t s) {
    hipLaunchKernelGGL(extract_expand_kernel, dim3(extract_blocks(a.n)), dim3(kExtractThreads), 0, s, a);
    return hipGetLastError();
}

}  // namespace vxrt
