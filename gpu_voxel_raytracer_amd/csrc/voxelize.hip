// voxelize.hip — device side of vxrt_voxelize.h: a triangle mesh in device memory -> the path keys and leaf words of the voxels its
// triangles meet, ready for the list builder's sort and dedupe (device_build.hip: sort_unique_list).  The host side is
// api_voxelize.hip; the rule, in exact integer arithmetic on vertices snapped to sixteenths of a voxel, is DESIGN.md §17.
//
//   setup     a thread per triangle: gather the three vertices (no index is followed before it is compared with n_verts), snap
//             them, take the candidate cells per axis and the columns along the normal's dominant axis -> tq[t], the block's
//             exclusive column offsets -> off[t], the block's columns -> part[block], its bounds and flags -> bounds[block]
//   reduce    one workgroup over the blocks' bounds -> 32 bytes read back
//   scan      part[] (device_build.h: launch_exclusive_scan)
//   offsets   off[t] += part[block of t]; off[n_tris] = W
//   walk      a thread per (triangle, column) item, the triangle found by binary search in the block's range of off[], staged in
//             LDS (an item has at least one column, so 256 items span at most 256 triangles).  The column's cells are cut to the
//             depth range the triangle's plane allows, by two exact 64-bit divisions, and each remaining cell takes the ten axis
//             tests.  Counting: the block's hits -> part[block].  Emitting: the hits' keys and leaf words at part[block] + the
//             thread's exclusive offset in the block; the first 64 cells' outcomes are kept in a mask between the count and the
//             writes, so a cell is tested once where the column is short, which it is along the dominant axis.
//   decode    a thread per unique key: the position and the (m & 0x7f, r, g, b) bytes
// 256 threads, no atomics: every position is a prefix sum in triangle order, then column order, then up the column.
#include "block_scan.h"
#include "ctx.h"
#include "device_build.h"
#include "voxelize.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kVoxThreads / 64;

__device__ __forceinline__ int64_t abs64(int64_t v) { return v < 0 ? -v : v; }

// rule 2: the candidate cells [*c0, *c1] of an axis whose snapped coordinates span [lo, hi]; a face on a cell boundary belongs to
// the cell above it only
__device__ __forceinline__ void cell_range(int lo, int hi, int* c0, int* c1) {
    *c0 = lo >> 4;
    *c1 = hi == lo ? *c0 : ((hi + 15) >> 4) - 1;
}

// A triangle as the walk sees it: the axes rotated (cyclically, so cross products rotate with them) so that the normal's dominant
// axis d is z and the columns run over x and y.  Original axis of x: (d + 1) % 3, of y: (d + 2) % 3.
struct Rotated {
    int q[3][3];          // [vertex][x, y, z]
    int64_t n[3];         // e0 x e1
    int c0[3], c1[3];     // candidate cells per axis
    int d;
};

__device__ __forceinline__ Rotated rotate(const int* q) {
    const int e0[3] = {q[3] - q[0], q[4] - q[1], q[5] - q[2]}, e1[3] = {q[6] - q[3], q[7] - q[4], q[8] - q[5]};
    const int64_t n0 = wmul(e0[1], e1[2]) - wmul(e0[2], e1[1]), n1 = wmul(e0[2], e1[0]) - wmul(e0[0], e1[2]),
                  n2 = wmul(e0[0], e1[1]) - wmul(e0[1], e1[0]);
    int d = 0;
    int64_t m = abs64(n0);
    if (abs64(n1) > m) { d = 1; m = abs64(n1); }      // the first axis of greatest |n_a|
    if (abs64(n2) > m) d = 2;
    Rotated r;
    r.d = d;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int x = q[3 * k], y = q[3 * k + 1], z = q[3 * k + 2];
        r.q[k][0] = d == 0 ? y : d == 1 ? z : x;
        r.q[k][1] = d == 0 ? z : d == 1 ? x : y;
        r.q[k][2] = d == 0 ? x : d == 1 ? y : z;
    }
    r.n[0] = d == 0 ? n1 : d == 1 ? n2 : n0;
    r.n[1] = d == 0 ? n2 : d == 1 ? n0 : n1;
    r.n[2] = d == 0 ? n0 : d == 1 ? n1 : n2;
#pragma unroll
    for (int ax = 0; ax < 3; ax++)
        cell_range(min3(r.q[0][ax], r.q[1][ax], r.q[2][ax]), max3(r.q[0][ax], r.q[1][ax], r.q[2][ax]), &r.c0[ax], &r.c1[ax]);
    return r;
}

// The three cross axes of one edge e, a = axis_i x e: the edge's two ends project to the same value, so the triangle's projection
// is spanned by one end (on) and the opposite vertex (opp), both relative to the cell's centre.  True: one of them separates.
__device__ __forceinline__ bool edge_separates(const int* e, const int* on, const int* opp) {
    bool sep = false;
    {   // axis x: a = (0, -e.z, e.y)
        const int64_t p0 = wmul(e[1], on[2]) - wmul(e[2], on[1]), p1 = wmul(e[1], opp[2]) - wmul(e[2], opp[1]);
        const int64_t r = 8 * (int64_t(abs(e[1])) + int64_t(abs(e[2])));
        sep |= min(p0, p1) > r || max(p0, p1) < -r;
    }
    {   // axis y: a = (e.z, 0, -e.x)
        const int64_t p0 = wmul(e[2], on[0]) - wmul(e[0], on[2]), p1 = wmul(e[2], opp[0]) - wmul(e[0], opp[2]);
        const int64_t r = 8 * (int64_t(abs(e[0])) + int64_t(abs(e[2])));
        sep |= min(p0, p1) > r || max(p0, p1) < -r;
    }
    {   // axis z: a = (-e.y, e.x, 0)
        const int64_t p0 = wmul(e[0], on[1]) - wmul(e[1], on[0]), p1 = wmul(e[0], opp[1]) - wmul(e[1], opp[0]);
        const int64_t r = 8 * (int64_t(abs(e[0])) + int64_t(abs(e[1])));
        sep |= min(p0, p1) > r || max(p0, p1) < -r;
    }
    return sep;
}

// rule 3 for the cell (cx, cy, cz) of the rotated triangle: the plane and the nine cross axes; touching is overlap
__device__ __forceinline__ bool cell_overlaps(const Rotated& t, int cx, int cy, int cz) {
    const int c[3] = {16 * cx + 8, 16 * cy + 8, 16 * cz + 8};
    int v[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int ax = 0; ax < 3; ax++) v[k][ax] = t.q[k][ax] - c[ax];
    const int64_t dist = t.n[0] * v[0][0] + t.n[1] * v[0][1] + t.n[2] * v[0][2];
    if (abs64(dist) > 8 * (abs64(t.n[0]) + abs64(t.n[1]) + abs64(t.n[2]))) return false;
    const int e0[3] = {t.q[1][0] - t.q[0][0], t.q[1][1] - t.q[0][1], t.q[1][2] - t.q[0][2]};
    const int e1[3] = {t.q[2][0] - t.q[1][0], t.q[2][1] - t.q[1][1], t.q[2][2] - t.q[1][2]};
    const int e2[3] = {t.q[0][0] - t.q[2][0], t.q[0][1] - t.q[2][1], t.q[0][2] - t.q[2][2]};
    return !(edge_separates(e0, v[0], v[2]) || edge_separates(e1, v[1], v[0]) || edge_separates(e2, v[2], v[1]));
}

// The cells [*z0, *z1] of column (cx, cy) that the plane test can pass: |s - 16 n_z c| <= r with s the plane's value at c = 0.
// Exact (floor and ceiling of the two quotients), so it drops no cell that rule 3 sets; an empty range has *z0 > *z1.
__device__ __forceinline__ void plane_range(const Rotated& t, int cx, int cy, int* z0, int* z1) {
    *z0 = t.c0[2];
    *z1 = t.c1[2];
    if (t.n[2] == 0) return;      // the dominant component: the normal is zero (a segment or a point), every cell is tested
    int64_t s = t.n[0] * (t.q[0][0] - (16 * cx + 8)) + t.n[1] * (t.q[0][1] - (16 * cy + 8)) + t.n[2] * (t.q[0][2] - 8);
    int64_t div = 16 * t.n[2];
    if (div < 0) { div = -div; s = -s; }
    const int64_t r = 8 * (abs64(t.n[0]) + abs64(t.n[1]) + abs64(t.n[2]));
    const int64_t a = s - r, b = s + r;
    int64_t lo = a / div, hi = b / div;
    if (a - lo * div > 0) lo++;       // ceiling
    if (b - hi * div < 0) hi--;       // floor
    *z0 = int(max(lo, int64_t(*z0)));
    *z1 = int(min(hi, int64_t(*z1)));
}

__global__ __launch_bounds__(kVoxThreads) void vox_setup_kernel(const float* verts, uint64_t n_verts, const uint32_t* tris, uint32_t n_tris, VoxTri* tq,
                                                                 uint64_t* off, uint64_t* part, MeshSummary* bounds) {
    __shared__ uint64_t lds[kWaves];
    const uint32_t t = blockIdx.x * kVoxThreads + threadIdx.x;
    BoxFlags v = empty_box();
    uint64_t columns = 0;
    if (t < n_tris) {
        int q[9];
        uint32_t flags = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const uint32_t idx = tris[3 * size_t(t) + k];
            const bool inside = idx < n_verts;
            if (!inside) flags |= kVoxBadIndex;
#pragma unroll
            for (int ax = 0; ax < 3; ax++) {
                const float f = inside ? verts[3 * size_t(idx) + ax] : 0.0f;
                if (!isfinite(f)) flags |= kVoxNotFinite;
                // rule 1: 16 f is exact in binary32 (or overflows to an infinity, which is outside), rintf rounds half to even
                const float r = isfinite(f) ? rintf(f * 16.0f) : 0.0f;
                if (!(r >= float(kVoxSnapLo) && r < float(kVoxSnapHi))) flags |= kVoxOutside;
                q[3 * k + ax] = int(fminf(fmaxf(r, -1073741824.0f), 1073741824.0f));
            }
        }
        VoxTri out{};
        if ((flags & (kVoxBadIndex | kVoxNotFinite)) == 0u) {
#pragma unroll
            for (int ax = 0; ax < 3; ax++)
                cell_range(min3(q[ax], q[3 + ax], q[6 + ax]), max3(q[ax], q[3 + ax], q[6 + ax]), &v.lo[ax], &v.hi[ax]);
            if (flags == 0u) {
                const Rotated r = rotate(q);
                columns = uint64_t(r.c1[0] - r.c0[0] + 1) * uint64_t(r.c1[1] - r.c0[1] + 1);
#pragma unroll
                for (int k = 0; k < 9; k++) out.q[k] = q[k];
            }
        }
        v.flags = flags;
        tq[t] = out;
    }
    uint64_t total;
    const uint64_t before = block_exclusive<uint64_t, kWaves>(columns, lds, &total);
    if (t < n_tris) off[t] = before;
    if (threadIdx.x == 0) part[blockIdx.x] = total;
    block_box_to<kWaves>(v, bounds + blockIdx.x);
}

__global__ __launch_bounds__(kVoxThreads) void vox_reduce_kernel(MeshSummary* bounds, uint32_t blocks) {
    BoxFlags v = empty_box();
    for (uint32_t k = threadIdx.x; k < blocks; k += kVoxThreads) {
        const MeshSummary b = bounds[k];
        merge(&v, BoxFlags{{b.lo[0], b.lo[1], b.lo[2]}, {b.hi[0], b.hi[1], b.hi[2]}, b.flags});
    }
    block_box_to<kWaves>(v, bounds + blocks);
}

// off[t]: within its block -> over the mesh; off[n_tris] = the total
__global__ __launch_bounds__(kVoxThreads) void vox_offsets_kernel(uint64_t* off, const uint64_t* part, uint32_t n_tris, uint32_t blocks) {
    const uint64_t t = uint64_t(blockIdx.x) * kVoxThreads + threadIdx.x;
    if (t < n_tris) off[t] += part[blockIdx.x];
    else if (t == n_tris) off[t] = part[blocks];
}

// kEmit false: part[block] = the block's hits.  kEmit true: part[block] is the hits before the block.
template <bool kEmit>
__global__ __launch_bounds__(kVoxThreads) void vox_walk_kernel(const VoxTri* tq, const uint64_t* off, uint32_t n_tris, uint32_t columns, uint64_t* part,
                                                                uint32_t depth, const uint8_t* tri_mrgb, uint64_t* keys, uint32_t* vals) {
    __shared__ uint64_t soff[kVoxThreads];
    __shared__ uint64_t lds[kWaves];
    const uint32_t g0 = blockIdx.x * kVoxThreads, g = g0 + threadIdx.x;     // blocks * 256 < 2^32 + 256: g0 < 2^32 as columns < 2^32
    // the last triangle whose items start at or before the block's first item (the same in every thread)
    uint32_t first = 0;
    for (uint32_t hi = n_tris - 1; first < hi;) {
        const uint32_t mid = first + (hi - first + 1) / 2;
        if (off[mid] <= g0) first = mid; else hi = mid - 1;
    }
    soff[threadIdx.x] = off[min(uint64_t(first) + threadIdx.x, uint64_t(n_tris))];
    __syncthreads();

    Rotated r{};
    uint32_t t = 0, count = 0;
    uint64_t mask = 0;      // the outcomes of the column's first 64 cells
    int cx = 0, cy = 0, z0 = 0, z1 = -1;
    if (g < columns) {
        uint32_t j = 0;
        for (uint32_t hi = kVoxThreads - 1; j < hi;) {      // off[first + 256] > g: every triangle has a column
            const uint32_t mid = j + (hi - j + 1) / 2;
            if (soff[mid] <= g) j = mid; else hi = mid - 1;
        }
        t = first + j;
        const uint32_t k = g - uint32_t(soff[j]);
        const uint4* src = reinterpret_cast<const uint4*>(tq + t);
        const uint4 a = src[0], b = src[1], c = src[2];
        const int q[9] = {int(a.x), int(a.y), int(a.z), int(a.w), int(b.x), int(b.y), int(b.z), int(b.w), int(c.x)};
        r = rotate(q);
        const uint32_t nx = uint32_t(r.c1[0] - r.c0[0] + 1);
        cx = r.c0[0] + int(k % nx);
        cy = r.c0[1] + int(k / nx);
        plane_range(r, cx, cy, &z0, &z1);
        for (int z = z0; z <= z1; z++) {
            const bool hit = cell_overlaps(r, cx, cy, z);
            if (kEmit && z - z0 < 64 && hit) mask |= uint64_t(1) << (z - z0);
            count += hit ? 1u : 0u;
        }
    }
    uint64_t total;
    const uint64_t before = block_exclusive<uint64_t, kWaves>(uint64_t(count), lds, &total);
    if (!kEmit) {
        if (threadIdx.x == 0) part[blockIdx.x] = total;
        return;
    }
    if (count == 0u) return;
    uint64_t at = part[blockIdx.x] + before;
    uint32_t word = 0u;
    if (vals) {
        const uint8_t* e = tri_mrgb + 4 * size_t(t);
        word = leaf_word_of(e[0], e[1], e[2], e[3]);
    }
    const int half = 1 << depth;
    for (int z = z0; z <= z1; z++) {
        const bool hit = z - z0 < 64 ? ((mask >> (z - z0)) & 1u) != 0u : cell_overlaps(r, cx, cy, z);
        if (!hit) continue;
        const int px = r.d == 0 ? z : r.d == 1 ? cy : cx, py = r.d == 0 ? cx : r.d == 1 ? z : cy, pz = r.d == 0 ? cy : r.d == 1 ? cx : z;
        keys[at] = path_key_of(uint32_t(px + half), uint32_t(py + half), uint32_t(pz + half), depth);
        if (vals) vals[at] = word;
        at++;
    }
}

__global__ __launch_bounds__(kVoxThreads) void vox_decode_kernel(const uint64_t* keys, const int32_t* words, uint32_t m, uint32_t depth, int16_t* pos,
                                                                  uint32_t* mrgb) {
    const uint32_t i = blockIdx.x * kVoxThreads + threadIdx.x;
    if (i >= m) return;
    const uint64_t key = keys[i];
    uint32_t u[3] = {0u, 0u, 0u};
    for (uint32_t k = 0; k <= depth; k++) {
        const uint32_t oct = uint32_t(key >> (3u * k)) & 7u;
        u[0] |= ((oct >> 2) & 1u) << k;
        u[1] |= ((oct >> 1) & 1u) << k;
        u[2] |= (oct & 1u) << k;
    }
    const int half = 1 << depth;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) pos[3 * size_t(i) + ax] = int16_t(int(u[ax]) - half);
    const uint32_t w = uint32_t(words[i]);      // 0x80 | m, r, g, b from the top byte down -> the bytes m & 0x7f, r, g, b in memory order
    mrgb[i] = ((w >> 24) & 0x7fu) | ((w >> 16) & 0xffu) << 8 | ((w >> 8) & 0xffu) << 16 | (w & 0xffu) << 24;
}

}  // namespace

int voxelize_setup(const float* verts, size_t n_verts, const uint32_t* tris, size_t n_tris, VoxTri* tq, uint64_t* off, uint64_t* part,
                   MeshSummary* bounds, hipStream_t s, MeshSummary* out, uint64_t* columns) {
    const uint32_t blocks = vox_blocks(n_tris), nt = uint32_t(n_tris);
    hipLaunchKernelGGL(vox_setup_kernel, dim3(blocks), dim3(kVoxThreads), 0, s, verts, uint64_t(n_verts), tris, nt, tq, off, part, bounds);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(vox_reduce_kernel, dim3(1), dim3(kVoxThreads), 0, s, bounds, blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_exclusive_scan(part, blocks, s));
    hipLaunchKernelGGL(vox_offsets_kernel, dim3(vox_blocks(uint64_t(n_tris) + 1)), dim3(kVoxThreads), 0, s, off, part, nt, blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, bounds + blocks, sizeof *out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(columns, part + blocks, sizeof *columns, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

int voxelize_count(const VoxTri* tq, const uint64_t* off, uint32_t n_tris, uint32_t columns, uint64_t* part, hipStream_t s, uint64_t* hits) {
    const uint32_t blocks = vox_blocks(columns);
    hipLaunchKernelGGL(vox_walk_kernel<false>, dim3(blocks), dim3(kVoxThreads), 0, s, tq, off, n_tris, columns, part, 0u, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_exclusive_scan(part, blocks, s));
    HIP_TRY(hipMemcpyAsync(hits, part + blocks, sizeof *hits, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

hipError_t voxelize_emit(const VoxTri* tq, const uint64_t* off, uint32_t n_tris, uint32_t columns, const uint64_t* part, uint32_t depth,
                         const uint8_t* tri_mrgb, uint64_t* keys, uint32_t* vals, hipStream_t s) {
    hipLaunchKernelGGL(vox_walk_kernel<true>, dim3(vox_blocks(columns)), dim3(kVoxThreads), 0, s, tq, off, n_tris, columns, const_cast<uint64_t*>(part),
                       depth, tri_mrgb, keys, vals);
    return hipGetLastError();
}

hipError_t voxelize_decode(const uint64_t* keys, const int32_t* words, uint32_t m, uint32_t depth, int16_t* pos, uint32_t* mrgb, hipStream_t s) {
    hipLaunchKernelGGL(vox_decode_kernel, dim3(vox_blocks(m)), dim3(kVoxThreads), 0, s, keys, words, m, depth, pos, mrgb);
    return hipGetLastError();
}

}  // namespace vxrt
