// transform_rule.h — rule 2 and rule 3 of include/vxrt_transform.h as the kernel runs them (transform.hip) and as a host compiler
// reads them (tests/test_transform_cpu.py builds a program of its own around this file): nothing from HIP is included, and the
// marker below is empty for a compiler that is not hipcc.  DESIGN.md §23.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VXRT_RULE_FN __host__ __device__ inline
#else
#define VXRT_RULE_FN inline
#endif

namespace vxrt {

// The source cell of destination cell d: per axis P = sum_j m[i][j] (2 d_j + 1) + 2 t[i] in 64 bits, s = P >> 17 (arithmetic: the
// floor), i.e. the cell that holds M (d + 1/2) + t.  With |m| <= 2^24, |t| <= 2^40 and |d| <= 2^15 every |P| is below 2^43.
VXRT_RULE_FN void pull_cell(const int32_t (*m)[3], const int64_t* t, const int32_t* d, int64_t* s) {
    const int64_t c0 = 2 * int64_t(d[0]) + 1, c1 = 2 * int64_t(d[1]) + 1, c2 = 2 * int64_t(d[2]) + 1;
    for (int i = 0; i < 3; i++) {
        const int64_t p = int64_t(m[i][0]) * c0 + int64_t(m[i][1]) * c1 + int64_t(m[i][2]) * c2 + 2 * t[i];
        s[i] = p >> 17;
    }
}

// A pulled centre is a source candidate only inside the int16 range, tested on the 64-bit values: with u = s + 32768 all three lie
// in [0, 65536) exactly when their union has no bit above bit 15 (a negative u has its high bits set).
VXRT_RULE_FN bool pull_in_range(const int64_t* s) {
    return uint64_t((s[0] + 32768) | (s[1] + 32768) | (s[2] + 32768)) < uint64_t(65536);
}

// Bit k of v (16 bits) to bit 3k.
VXRT_RULE_FN uint64_t spread16(uint32_t v) {
    uint64_t x = v & 0xffffu;
    x = (x | x << 16) & 0x0000ff0000ffull;
    x = (x | x << 8) & 0x00f00f00f00full;
    x = (x | x << 4) & 0x0c30c30c30c3ull;
    x = (x | x << 2) & 0x249249249249ull;
    return x;
}

// The path key at depth 15 of the cell (x, y, z) of the int16 range (device_build.h: path_key_of(u, 15), u = cell + 32768): 48 bits.
VXRT_RULE_FN uint64_t path_key15(int32_t x, int32_t y, int32_t z) {
    return spread16(uint32_t(x + 32768)) << 2 | spread16(uint32_t(y + 32768)) << 1 | spread16(uint32_t(z + 32768));
}

}  // namespace vxrt
