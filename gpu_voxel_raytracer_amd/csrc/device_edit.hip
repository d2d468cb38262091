// device_edit.hip — device side of vxrt_device_edit.h: the one pass over a voxel list in device memory that vxrt_edit_voxels_device
// needs before the shared sort, dedupe and cut (device_build.hip, grid_edit.hip).  The host side is api_device_edit.hip; DESIGN.md §15.
//
//   keys     a thread per 8 consecutive entries: the path key at the scene's depth (device_build.h: path_key_of, the key
//            vxrt_edit_voxels sorts by) and, for a set, the leaf word; the thread's least and greatest position per axis and whether
//            one of its positions lies outside the root cube -> reduced per block (block_scan.h: block_box_to) -> part[block]
//   reduce   one workgroup over the blocks' partials -> 32 bytes read back
// Where the arrays are 16-byte aligned a thread reads its 48 bytes of positions as three 16-byte loads and its 32 bytes of mrgb as two;
// otherwise, and for the list's last entries when n is no multiple of 8, element by element.  Nothing is decided by an atomic.
#include "block_scan.h"
#include "ctx.h"
#include "device_build.h"
#include "edit.h"

namespace vxrt {
namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kGroup = 8;                      // entries per thread
constexpr uint32_t kSpan = kThreads * kGroup;       // entries per block

// vec_pos / vec_mrgb: the array is 16-byte aligned.  mrgb == nullptr (a clear): no leaf words, vals is not touched.
__global__ __launch_bounds__(kThreads) void edit_keys_kernel(const int16_t* pos, const uint8_t* mrgb, size_t n, uint32_t depth, uint32_t vec_pos,
                                                              uint32_t vec_mrgb, uint64_t* keys, uint32_t* vals, ListBounds* part) {
    const size_t i0 = (size_t(blockIdx.x) * kThreads + threadIdx.x) * kGroup;
    BoxFlags v = empty_box();
    if (i0 < n) {
        const bool full = n - i0 >= kGroup;
        const uint32_t count = full ? kGroup : uint32_t(n - i0);
        int p[3 * kGroup];
        uint32_t w[kGroup];   // mrgb bytes, the material lowest
        if (full && vec_pos) {
            const uint4* q = reinterpret_cast<const uint4*>(pos + 3 * i0);   // 48 i0 bytes from an aligned base
#pragma unroll
            for (uint32_t k = 0; k < 3; k++) {
                const uint4 t = q[k];
                const uint32_t h[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (uint32_t j = 0; j < 4; j++) {
                    p[8 * k + 2 * j + 0] = int(int16_t(h[j] & 0xffffu));
                    p[8 * k + 2 * j + 1] = int(int16_t(h[j] >> 16));
                }
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 3 * kGroup; k++) p[k] = k < 3 * count ? int(pos[3 * i0 + k]) : 0;
        }
        if (mrgb) {
            if (full && vec_mrgb) {
                const uint4* q = reinterpret_cast<const uint4*>(mrgb + 4 * i0);
                const uint4 a = q[0], b = q[1];
                w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
                w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < kGroup; k++) {
                    const uint8_t* e = mrgb + 4 * (i0 + k);
                    w[k] = k < count ? uint32_t(e[0]) | uint32_t(e[1]) << 8 | uint32_t(e[2]) << 16 | uint32_t(e[3]) << 24 : 0u;
                }
            }
        }
        const int half = 1 << depth;
#pragma unroll
        for (uint32_t k = 0; k < kGroup; k++) {
            if (k < count) {
                uint32_t u[3];
#pragma unroll
                for (int ax = 0; ax < 3; ax++) {
                    const int c = p[3 * k + ax];
                    v.lo[ax] = min(v.lo[ax], c);
                    v.hi[ax] = max(v.hi[ax], c);
                    v.flags |= (c < -half || c >= half) ? 1u : 0u;      // ListBounds::outside
                    u[ax] = uint32_t(c + half);
                }
                keys[i0 + k] = path_key_of(u[0], u[1], u[2], depth);   // of an outside position: never used, the call is refused
                if (mrgb) vals[i0 + k] = leaf_word_of(w[k] & 0xffu, (w[k] >> 8) & 0xffu, (w[k] >> 16) & 0xffu, w[k] >> 24);
            }
        }
    }
    block_box_to<kWaves>(v, part + blockIdx.x);
}

__global__ __launch_bounds__(kThreads) void edit_bounds_reduce_kernel(ListBounds* part, uint32_t blocks) {
    BoxFlags v = empty_box();
    for (uint32_t k = threadIdx.x; k < blocks; k += kThreads) {
        const ListBounds b = part[k];
        merge(&v, BoxFlags{{b.lo[0], b.lo[1], b.lo[2]}, {b.hi[0], b.hi[1], b.hi[2]}, b.outside});
    }
    block_box_to<kWaves>(v, part + blocks);
}

}  // namespace

int edit_keys_device(const int16_t* pos, const uint8_t* mrgb, size_t n, uint32_t depth, uint64_t* keys, uint32_t* vals, hipStream_t s,
                     const char* who, ListBounds* out) {
    const uint32_t blocks = uint32_t((n + kSpan - 1) / kSpan);   // n < 2^32
    ScratchBuffer part;
    if (int rc = alloc_scratch(&part, (size_t(blocks) + 1) * sizeof(ListBounds), who, "the bounds")) return rc;
    const uint32_t vec_pos = (reinterpret_cast<uintptr_t>(pos) & 15u) == 0u ? 1u : 0u;
    const uint32_t vec_mrgb = (reinterpret_cast<uintptr_t>(mrgb) & 15u) == 0u ? 1u : 0u;
    hipLaunchKernelGGL(edit_keys_kernel, dim3(blocks), dim3(kThreads), 0, s, pos, mrgb, n, depth, vec_pos, vec_mrgb, keys, vals,
                       part.as<ListBounds>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(edit_bounds_reduce_kernel, dim3(1), dim3(kThreads), 0, s, part.as<ListBounds>(), blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, part.as<ListBounds>() + blocks, sizeof *out, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
}

}  // namespace vxrt
