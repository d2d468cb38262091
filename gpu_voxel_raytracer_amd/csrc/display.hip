// display.hip — the displayed frame: VXRT_DENOISED encoded to 8-bit sRGB, 4 bytes per pixel (include/vxrt.h: VXRT_DISPLAY_*).
// The reference shows denoised_color through a Bgra8UnormSrgb swap chain (src/context.rs:663, 696-706; shaders/display.frag maps pixels
// one to one), and Vulkan leaves the rounding of an sRGB store to the implementation.  The library fixes one rule:
//   colour channel:  NaN, x <= 0 -> 0;  x >= 1 -> 255;  otherwise round_half_up(255 * S(x)) evaluated exactly,
//                    S(x) = 12.92 x (x <= 0.0031308), 1.055 x^(1/2.4) - 0.055 otherwise
//   alpha:           round_half_up(255 * clamp(a, 0, 1)), NaN -> 0 (linear)
// The colour byte is a monotone step function of x, so it equals the number of the 255 binary32 thresholds T[k] (the smallest float
// whose byte is >= k + 1) that are <= x — which also gives NaN, -0, the infinities and negative values their bytes without a special
// case.  The host makes T once by bisection over float bit patterns with the formula in binary64 (no binary32 input comes within
// 2.2e-9 of a step of a half-step, so binary64 rounds every one of them correctly); the kernel counts with an 8-step binary search in
// LDS — no transcendental per element, so the kernel stays memory-bound.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/vxrt.h"
#include "../../include/vxrt_debug.h"
#include "kernels.h"
#include "scene_host.h"

namespace vxrt {

namespace {

// the rule in binary64, specials first (the test oracle restates it in numpy)
int display_byte_f64(float xf) {
    if (std::isnan(xf) || xf <= 0.0f) return 0;
    if (xf >= 1.0f) return 255;
    const double x = double(xf);
    const double s = x <= 0.0031308 ? 12.92 * x : 1.055 * std::pow(x, 1.0 / 2.4) - 0.055;
    return int(std::floor(255.0 * s + 0.5));
}

struct Thresholds {
    DisplayTable t{};
    Thresholds() {
        // T[k]: the smallest positive float whose byte is >= k + 1 (bit patterns of non-negative floats order like their values)
        for (int k = 0; k < 255; k++) {
            uint32_t lo = 0u, hi = 0x3f800000u;      // byte(0) = 0 < k + 1 <= 255 = byte(1)
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                float f;
                std::memcpy(&f, &mid, 4);
                if (display_byte_f64(f) >= k + 1) hi = mid; else lo = mid;
            }
            std::memcpy(&t.t[k], &hi, 4);
        }
        t.t[255] = INFINITY;   // padding: loaded into LDS with the rest, never compared
    }
};

const DisplayTable& thresholds() {
    static const Thresholds th;    // made once per process, thread-safe
    return th.t;
}

// colour byte = #{k : T[k] <= x}: 8 branchless halvings over the 255 sorted thresholds (indices 0 .. 254 are read; NaN compares false
// everywhere and counts 0)
__device__ __forceinline__ uint32_t srgb_byte(float x, const float* t) {
    uint32_t k = 0u;
#pragma unroll
    for (uint32_t step = 128u; step >= 1u; step >>= 1)
        k += (t[k + step - 1u] <= x) ? step : 0u;
    return k;
}

// alpha byte: round_half_up(255 a), exact in binary64 (a 24-bit significand times 255 needs 32 bits)
__device__ __forceinline__ uint32_t alpha_byte(float a) {
    if (!(a > 0.0f)) return 0u;           // NaN, -0, negative
    if (a >= 1.0f) return 255u;
    return uint32_t(floor(double(a) * 255.0 + 0.5));
}

template <bool BGRA>
__device__ __forceinline__ uint32_t encode_pixel(float4 v, const float* t) {
    const uint32_t r = srgb_byte(v.x, t), g = srgb_byte(v.y, t), b = srgb_byte(v.z, t), a = alpha_byte(v.w);
    return BGRA ? (b | (g << 8) | (r << 16) | (a << 24)) : (r | (g << 8) | (b << 16) | (a << 24));
}

constexpr int kDisplayBlock = 256;
constexpr unsigned kDisplayMaxBlocks = 2048;

}  // namespace

// One lane: 4 consecutive pixels = four 16-byte loads and one 16-byte store; a grid of at most 2048 blocks strides over the rest.
// The n % 4 pixels of the tail go to the first lanes of the grid, one each.  Named for rocprofv3: vxrt::display_encode_kernel<bool>.
template <bool BGRA>
__global__ __launch_bounds__(kDisplayBlock) void display_encode_kernel(const float4* __restrict__ src, uint32_t* __restrict__ dst,
                                                                       size_t n, DisplayTable tab) {
    __shared__ float t[256];
    t[threadIdx.x] = tab.t[threadIdx.x];
    __syncthreads();
    const size_t n4 = n / 4u;
    const size_t first = size_t(blockIdx.x) * kDisplayBlock + threadIdx.x;
    const size_t stride = size_t(gridDim.x) * kDisplayBlock;
    for (size_t q = first; q < n4; q += stride) {
        const float4 p0 = src[4u * q], p1 = src[4u * q + 1u], p2 = src[4u * q + 2u], p3 = src[4u * q + 3u];
        uint4 o;
        o.x = encode_pixel<BGRA>(p0, t);
        o.y = encode_pixel<BGRA>(p1, t);
        o.z = encode_pixel<BGRA>(p2, t);
        o.w = encode_pixel<BGRA>(p3, t);
        reinterpret_cast<uint4*>(dst)[q] = o;
    }
    if (first < n - 4u * n4) dst[4u * n4 + first] = encode_pixel<BGRA>(src[4u * n4 + first], t);
}

hipError_t launch_display_encode(const float4* src, uint32_t* dst, size_t n, bool bgra, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const size_t want = (n / 4u + kDisplayBlock - 1) / kDisplayBlock;
    const unsigned blocks = unsigned(want == 0 ? 1 : (want < kDisplayMaxBlocks ? want : kDisplayMaxBlocks));
    if (bgra)
        hipLaunchKernelGGL(display_encode_kernel<true>, dim3(blocks), dim3(kDisplayBlock), 0, s, src, dst, n, thresholds());
    else
        hipLaunchKernelGGL(display_encode_kernel<false>, dim3(blocks), dim3(kDisplayBlock), 0, s, src, dst, n, thresholds());
    return hipGetLastError();
}

}  // namespace vxrt

extern "C" int vxrt_display_thresholds(float out[255]) {
    if (!out) { vxrt::set_error("null argument"); return VXRT_E_INVALID; }
    std::memcpy(out, vxrt::thresholds().t, 255 * sizeof(float));
    return VXRT_OK;
}
