// block_scan.h — wave and workgroup reductions and prefix sums (wave64) shared by the level-synchronous kernels (extract.hip,
// device_build.hip, edit.hip, device_edit.hip, voxelize.hip, components.hip, pieces.hip, query.hip) and the list operators'
// (run_heads.hip, morph.hip, mesh.hip, distance.hip).  Everything is in thread order
// and integer, so the results never depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace vxrt {

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

template <typename T> __device__ __forceinline__ T wave_inclusive(T v, uint32_t lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T up = __shfl_up(v, off, 64);
        if (lane >= uint32_t(off)) v += up;
    }
    return v;
}

// exclusive prefix sum of v over the block of W waves (in thread order); *total = the block's sum.  Ends with a barrier.
template <typename T, uint32_t W> __device__ __forceinline__ T block_exclusive(T v, T* lds, T* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const T incl = wave_inclusive(v, lane);
    if (lane == 63u) lds[wave] = incl;
    __syncthreads();
    T before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; w++) {
        const T t = lds[w];
        if (w < wave) before += t;
        all += t;
    }
    *total = all;
    __syncthreads();
    return before + incl - v;
}

// the sum of `mine` over the block of W waves -> *out (thread 0 writes; per-wave sums, added in wave order).  Once per kernel: its
// LDS is not reused, and no barrier follows the read.
template <uint32_t W, typename Out> __device__ __forceinline__ void block_sum_to(uint32_t mine, Out* out) {
    __shared__ uint32_t lds[W];
    mine = wave_sum(mine);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < W; w++) all += lds[w];
        *out = all;
    }
}

// The two halves of a compaction over a block of W waves, kItems <= 32 items per thread side by side: bit k of `kept` says that
// the thread keeps its item k.  Counting (kEmit == false): the block's kept items -> part[blockIdx.x] (block_sum_to: once per
// kernel).  Emitting (part scanned): write(k, to) for every kept item in item order, `to` counting up from part[blockIdx.x] plus
// what the threads before this one keep, so that a block's output stands in the order of its input.
template <uint32_t W, uint32_t kItems, bool kEmit, typename Part, typename Write>
__device__ __forceinline__ void block_compact(uint32_t kept, Part* part, Write write) {
    const uint32_t mine = uint32_t(__builtin_popcount(kept));
    if constexpr (!kEmit) {
        block_sum_to<W>(mine, part + blockIdx.x);
    } else {
        __shared__ uint32_t scan[W];
        uint32_t all;
        uint64_t to = part[blockIdx.x] + block_exclusive<uint32_t, W>(mine, scan, &all);
#pragma unroll
        for (uint32_t k = 0; k < kItems; k++) {
            if (kept >> k & 1u) {
                write(k, to);
                to++;
            }
        }
    }
}

// A box and flag bits: what the passes over a voxel list (device_edit.hip) and over a mesh (voxelize.hip) reduce.
struct BoxFlags {
    int lo[3], hi[3];
    uint32_t flags;
};

__device__ __forceinline__ BoxFlags empty_box() { return BoxFlags{{INT_MAX, INT_MAX, INT_MAX}, {INT_MIN, INT_MIN, INT_MIN}, 0u}; }

__device__ __forceinline__ void merge(BoxFlags* a, const BoxFlags& b) {
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        a->lo[ax] = min(a->lo[ax], b.lo[ax]);
        a->hi[ax] = max(a->hi[ax], b.hi[ax]);
    }
    a->flags |= b.flags;
}

// the block's box and flags (W waves) -> *out (thread 0 writes), a record of lo[3], hi[3], the flags and a pad word (edit.h:
// ListBounds, voxelize.h: MeshSummary).  Once per kernel, as block_sum_to.
template <uint32_t W, typename Rec> __device__ __forceinline__ void block_box_to(BoxFlags v, Rec* out) {
    __shared__ BoxFlags lds[W];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        BoxFlags o;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            o.lo[ax] = __shfl_xor(v.lo[ax], off, 64);
            o.hi[ax] = __shfl_xor(v.hi[ax], off, 64);
        }
        o.flags = uint32_t(__shfl_xor(int(v.flags), off, 64));
        merge(&v, o);
    }
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < W; w++) merge(&v, lds[w]);
        *out = Rec{{v.lo[0], v.lo[1], v.lo[2]}, {v.hi[0], v.hi[1], v.hi[2]}, v.flags, 0u};
    }
}

}  // namespace vxrt
