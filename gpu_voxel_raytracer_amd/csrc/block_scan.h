// block_scan.h — wave and workgroup reductions and prefix sums (wave64) shared by the level-synchronous kernels (extract.hip,
// device_build.hip).  Everything is in thread order and integer, so the results never depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace vxrt {

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
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

}  // namespace vxrt
