// run_heads.hip — run_heads.h's kernel: the first entry of each run of keys[i] >> shift in a sorted key array, counted per block and
// written in the order of the input.
//
// Unique result: every word written is a function of the keys, the words and the shift alone; the counts are integer sums in
// thread order.  Bounds: a thread takes kMorphItems entries side by side and loads each once, and the entry before its first,
// unconditionally from an index clamped into the array (at_of); every store sits at an offset the counting pass summed; no workgroup
// waits for another, and there is no atomic.
#include "run_heads.h"

#include "block_scan.h"
#include "morph.h"

namespace vxrt {
namespace {

template <bool kEmit>
__global__ __launch_bounds__(kMorphThreads) void run_heads_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ words,
                                                                  const uint32_t n, const uint32_t shift, uint64_t* __restrict__ part,
                                                                  uint64_t* __restrict__ out_keys, uint32_t* __restrict__ out_words) {
    const bool with_words = kEmit && words != nullptr && out_words != nullptr;      // uniform over the grid
    uint64_t before = keys[at_of(item_beside(0) - 1u, n)];      // wraps at entry 0: clamped, and not used
    uint64_t key[kMorphItems];
    uint32_t word[kMorphItems], heads = 0;
#pragma unroll
    for (uint32_t k = 0; k < kMorphItems; k++) {
        const uint64_t i = item_beside(k);
        key[k] = keys[at_of(i, n)];
        word[k] = with_words ? words[at_of(i, n)] : 0u;
        heads |= (run_is_head(key[k], before, i, n, shift) ? 1u : 0u) << k;
        before = key[k];
    }
    block_compact<kMorphThreads / 64, kMorphItems, kEmit>(heads, part, [&](uint32_t k, uint64_t to) {
        out_keys[to] = key[k] >> shift;
        if (with_words) out_words[to] = word[k];
    });
}

}  // namespace

hipError_t launch_run_heads(const uint64_t* keys, const uint32_t* words, uint32_t n, uint32_t shift, uint64_t* part, uint64_t* out_keys,
                            uint32_t* out_words, hipStream_t stream) {
    const dim3 grid(morph_blocks(n)), block(kMorphThreads);
    if (out_keys != nullptr)
        hipLaunchKernelGGL(run_heads_kernel<true>, grid, block, 0, stream, keys, words, n, shift, part, out_keys, out_words);
    else
        hipLaunchKernelGGL(run_heads_kernel<false>, grid, block, 0, stream, keys, words, n, shift, part, out_keys, out_words);
    return hipGetLastError();
}

}  // namespace vxrt
