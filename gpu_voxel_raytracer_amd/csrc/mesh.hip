// mesh.hip — device side of vxrt_mesh.h: the exposed faces of a sorted unique key array counted and written as sortable face keys
// (mesh_face_count_kernel, mesh_face_emit_kernel), the heads of the runs among the sorted faces (mesh_heads_kernel), each quad's
// four corner keys (mesh_quad_corners_kernel), and the two kernels that write the caller's arrays (mesh_triangles_kernel,
// mesh_vertices_kernel); the distinct corners are the run heads of the sorted corner keys (run_heads.hip).  The thread's items
// (item_beside, item_apart, at_of) are morph.h's, the compaction block_scan.h's.  The host side is api_mesh.hip; the face
// key, the head test, the corners and the index walk are mesh_rule.h's, the kernels' contracts are in mesh.h and the argument in
// DESIGN.md §27.
//
// Unique result: every word written is a function of the key array, its words and the mode alone; the counts are integer sums in
// thread order.  Bounds: every loop runs a fixed count (kMorphItems items, 6 directions, 4 corners, at most 32 steps of the walk);
// every load is unconditional from an index clamped into its array (morph_safe_index), every store sits behind the test of its
// own index against the array's count or at an offset the counting pass summed; no workgroup waits for another, and there is no
// atomic.
#include "block_scan.h"
#include "mesh.h"

namespace vxrt {
namespace {

constexpr uint32_t kWaves = kMorphThreads / 64;

__global__ __launch_bounds__(kMorphThreads) void mesh_face_count_kernel(const uint32_t* __restrict__ masks, const uint32_t m,
                                                                        uint64_t* __restrict__ part) {
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint64_t i = item_apart(k);
        const uint32_t mask = masks[at_of(i, m)];
        mine += i < m ? uint32_t(__builtin_popcount(mesh_face_dirs(mask))) : 0u;
    }
    block_sum_to<kWaves>(mine, part + blockIdx.x);
}

__global__ __launch_bounds__(kMorphThreads) void mesh_face_emit_kernel(const MorphSet s, const uint32_t* __restrict__ masks,
                                                                       const uint64_t* __restrict__ part, uint64_t* __restrict__ out_faces,
                                                                       uint32_t* __restrict__ out_words) {
    uint64_t key[kMorphItems];
    uint32_t word[kMorphItems], dirs[kMorphItems], mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint64_t i = item_beside(k);
        const uint32_t at = at_of(i, s.m);
        key[k] = s.keys[at];
        word[k] = out_words != nullptr ? s.words[at] : 0u;      // uniform over the grid
        dirs[k] = i < s.m ? mesh_face_dirs(masks[at]) : 0u;
        mine += uint32_t(__builtin_popcount(dirs[k]));
    }
    __shared__ uint32_t scan[kWaves];
    uint32_t all;
    uint64_t to = part[blockIdx.x] + block_exclusive<uint32_t, kWaves>(mine, scan, &all);
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
#pragma unroll
        for (uint32_t d = 0; d < kMeshDirs; d++) {
            if (dirs[k] >> d & 1u) {
                out_faces[to] = mesh_face_of(key[k], d);
                if (out_words != nullptr) out_words[to] = word[k];
                to++;
            }
        }
    }
}

template <bool kEmit>
__global__ __launch_bounds__(kMorphThreads) void mesh_heads_kernel(const uint64_t* __restrict__ faces, const uint32_t* __restrict__ words,
                                                                   const uint32_t count, const uint32_t mode, uint64_t* __restrict__ part,
                                                                   uint32_t* __restrict__ out_heads) {
    uint32_t heads = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint64_t i = item_beside(k);
        const uint32_t at = at_of(i, count), before = at_of(i - 1u, count);      // wraps at i == 0: clamped, and not used
        const uint64_t cur = faces[at], prev = faces[before];
        const uint32_t cur_word = words != nullptr ? words[at] : 0u, prev_word = words != nullptr ? words[before] : 0u;
        heads |= (i < count && mesh_is_head(prev, prev_word, cur, cur_word, i == 0u, mode, words != nullptr) ? 1u : 0u) << k;
    }
    block_compact<kWaves, kMorphItems, kEmit>(heads, part, [&](uint32_t k, uint64_t to) { out_heads[to] = uint32_t(item_beside(k)); });
}

// Quad j as its first face and its length: heads[j] and the distance to the next head (the last quad ends at `count`).
struct Quad {
    uint64_t face;
    uint32_t head, len;
};
__device__ __forceinline__ Quad load_quad(const uint64_t* __restrict__ faces, uint32_t count, const uint32_t* __restrict__ heads, uint32_t quads,
                                          uint64_t j) {
    const uint32_t head = heads[at_of(j, quads)], next = heads[at_of(j + 1u, quads)];
    const uint32_t end = j + 1u < quads ? next : count;
    return Quad{faces[morph_safe_index(head, count)], head, end - head};
}

__global__ __launch_bounds__(kMorphThreads) void mesh_quad_corners_kernel(const uint64_t* __restrict__ faces, const uint32_t count,
                                                                          const uint32_t* __restrict__ heads, const uint32_t quads,
                                                                          uint64_t* __restrict__ out_corners) {
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint64_t j = item_apart(k);
        const Quad q = load_quad(faces, count, heads, quads, j);
        const MeshCorners c = mesh_quad_corners(q.face, q.len);
        if (j < quads) {
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) out_corners[4u * size_t(j) + i] = c.k[i];
        }
    }
}

// One quad at a time per thread, its four corners walked side by side: the four probes of a step are loaded, whatever the corners
// are, and taken behind one wait (morph.hip's walk).  A lane past the last quad walks the last quad's corners and writes nothing.
__global__ __launch_bounds__(kMorphThreads) void mesh_triangles_kernel(const uint64_t* __restrict__ faces, const uint32_t* __restrict__ words,
                                                                       const uint32_t count, const uint32_t* __restrict__ heads,
                                                                       const uint32_t quads, const uint64_t* __restrict__ verts,
                                                                       const uint32_t n_verts, const uint32_t steps, uint32_t* out_tris,
                                                                       uint8_t* out_mrgb) {
#pragma unroll 1
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint64_t j = item_apart(k);
        const Quad q = load_quad(faces, count, heads, quads, j);
        const uint32_t word = out_mrgb != nullptr ? words[morph_safe_index(q.head, count)] : 0u;      // uniform over the grid
        const MeshCorners c = mesh_quad_corners(q.face, q.len);
        uint32_t at[4] = {0u, 0u, 0u, 0u};
        uint64_t probed[4];
#pragma unroll 1
        for (uint32_t left = steps; left != 0u; left--) {
            const uint64_t step = uint64_t(1) << (left - 1u);
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) probed[i] = verts[list_index(walk_probe(at[i], step), n_verts)];
            __builtin_amdgcn_sched_barrier(0);      // all four reads are out before the first is waited for
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) at[i] = walk_take(probed[i], c.k[i], at[i], step, list_there(walk_probe(at[i], step), n_verts));
        }
        if (j < quads) {
            uint32_t* t = out_tris + 6u * size_t(j);
            t[0] = at[0];
            t[1] = at[1];
            t[2] = at[2];
            t[3] = at[0];
            t[4] = at[2];
            t[5] = at[3];
            if (out_mrgb != nullptr) {
                uint8_t* b = out_mrgb + 8u * size_t(j);
#pragma unroll
                for (uint32_t tri = 0; tri < 2u; tri++) {
                    b[4u * tri] = uint8_t((word >> 24) & 0x7fu);
                    b[4u * tri + 1u] = uint8_t((word >> 16) & 0xffu);
                    b[4u * tri + 2u] = uint8_t((word >> 8) & 0xffu);
                    b[4u * tri + 3u] = uint8_t(word & 0xffu);
                }
            }
        }
    }
}

__global__ __launch_bounds__(kMorphThreads) void mesh_vertices_kernel(const uint64_t* __restrict__ verts, const uint32_t n_verts, float* out_verts) {
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint64_t i = item_apart(k);
        const MeshVertex v = mesh_corner_vertex(verts[at_of(i, n_verts)]);
        if (i < n_verts) {
            float* o = out_verts + 3u * size_t(i);
            o[0] = v.v[0];
            o[1] = v.v[1];
            o[2] = v.v[2];
        }
    }
}

}  // namespace

hipError_t launch_mesh_face_count(const uint32_t* masks, uint32_t m, uint64_t* part, hipStream_t stream) {
    hipLaunchKernelGGL(mesh_face_count_kernel, dim3(morph_blocks(m)), dim3(kMorphThreads), 0, stream, masks, m, part);
    return hipGetLastError();
}

hipError_t launch_mesh_face_emit(const MorphSet& s, const uint32_t* masks, const uint64_t* part, uint64_t* out_faces, uint32_t* out_words,
                                 hipStream_t stream) {
    hipLaunchKernelGGL(mesh_face_emit_kernel, dim3(morph_blocks(s.m)), dim3(kMorphThreads), 0, stream, s, masks, part, out_faces, out_words);
    return hipGetLastError();
}

hipError_t launch_mesh_heads(const uint64_t* faces, const uint32_t* words, uint32_t count, uint32_t mode, uint64_t* part, uint32_t* out_heads,
                             hipStream_t stream) {
    const dim3 grid(morph_blocks(count)), block(kMorphThreads);
    if (out_heads != nullptr)
        hipLaunchKernelGGL(mesh_heads_kernel<true>, grid, block, 0, stream, faces, words, count, mode, part, out_heads);
    else
        hipLaunchKernelGGL(mesh_heads_kernel<false>, grid, block, 0, stream, faces, words, count, mode, part, out_heads);
    return hipGetLastError();
}

hipError_t launch_mesh_quad_corners(const uint64_t* faces, uint32_t count, const uint32_t* heads, uint32_t quads, uint64_t* out_corners,
                                    hipStream_t stream) {
    hipLaunchKernelGGL(mesh_quad_corners_kernel, dim3(morph_blocks(quads)), dim3(kMorphThreads), 0, stream, faces, count, heads, quads, out_corners);
    return hipGetLastError();
}

hipError_t launch_mesh_triangles(const uint64_t* faces, const uint32_t* words, uint32_t count, const uint32_t* heads, uint32_t quads,
                                 const uint64_t* verts, uint32_t n_verts, uint32_t* out_tris, uint8_t* out_mrgb, hipStream_t stream) {
    hipLaunchKernelGGL(mesh_triangles_kernel, dim3(morph_blocks(quads)), dim3(kMorphThreads), 0, stream, faces, words, count, heads, quads, verts,
                       n_verts, list_steps(n_verts), out_tris, out_mrgb);
    return hipGetLastError();
}

hipError_t launch_mesh_vertices(const uint64_t* verts, uint32_t n_verts, float* out_verts, hipStream_t stream) {
    hipLaunchKernelGGL(mesh_vertices_kernel, dim3(morph_blocks(n_verts)), dim3(kMorphThreads), 0, stream, verts, n_verts, out_verts);
    return hipGetLastError();
}

}  // namespace vxrt
