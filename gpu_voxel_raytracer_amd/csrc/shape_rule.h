// shape_rule.h — rules 1 to 3 of include/vxrt_shape.h as the kernels run them (shape.hip) and as a host compiler reads them
// (tests/test_shape_cpu.py builds a program of its own around this file): nothing from HIP is included; the marker, spread16 and
// path_key15 are transform_rule.h's.  DESIGN.md §29.
#pragma once
#include "transform_rule.h"

namespace vxrt {

constexpr uint32_t kShapeBox = 0, kShapeBall = 1, kShapeCylinder = 2, kShapeCapsule = 3;   // vxrt_shape_kind

// Rule 1: the pulled centre of destination cell d in units of 2^-17 cell: per axis P = sum_j m[i][j] (2 d_j + 1) + 2 t[i] in 64
// bits, pull_cell's sum before its shift.  With |m| <= 2^24, |t| <= 2^40 and |d| <= 2^15 every |P| is below 2^43.
VXRT_RULE_FN void shape_pull(const int32_t (*m)[3], const int64_t* t, const int32_t* d, int64_t* p) {
    const int64_t c0 = 2 * int64_t(d[0]) + 1, c1 = 2 * int64_t(d[1]) + 1, c2 = 2 * int64_t(d[2]) + 1;
    // written out, not looped: a loop the compiler leaves rolled indexes p and m by a register, which puts them in scratch
    p[0] = int64_t(m[0][0]) * c0 + int64_t(m[0][1]) * c1 + int64_t(m[0][2]) * c2 + 2 * t[0];
    p[1] = int64_t(m[1][0]) * c0 + int64_t(m[1][1]) * c1 + int64_t(m[1][2]) * c2 + 2 * t[1];
    p[2] = int64_t(m[2][0]) * c0 + int64_t(m[2][1]) * c1 + int64_t(m[2][2]) * c2 + 2 * t[2];
}

// Rule 2: every |P_i| < 2^31, tested on the 64-bit values: with b = 2^31 - 1 the six values b + P_i and b - P_i all lie in
// [0, 2^32) exactly when every P_i lies in [-b, b], and they do exactly when their union has no bit above bit 31 (a negative value
// has its high bits set).
VXRT_RULE_FN bool shape_near(const int64_t* p) {
    const int64_t b = (int64_t(1) << 31) - 1;
    return uint64_t((b + p[0]) | (b + p[1]) | (b + p[2]) | (b - p[0]) | (b - p[1]) | (b - p[2])) < (uint64_t(1) << 32);
}

// v^2 for |v| < 2^31: below 2^62.  One 32 x 32 -> 64 bit product.
VXRT_RULE_FN uint64_t shape_square(int64_t v) {
    const int64_t w = int64_t(int32_t(v));
    return uint64_t(w * w);
}

// Rule 3 for a centre that passed rule 2: r2 = 2 r, h2[i] = 2 h[i] (r, h <= 2^29: r2^2 <= 2^60, and three squares below 2^62 do not
// wrap 64 unsigned bits).
VXRT_RULE_FN bool shape_holds(uint32_t kind, int64_t r2, const int64_t* h2, const int64_t* p) {
    const uint64_t rr = uint64_t(r2) * uint64_t(r2);
    const uint64_t xy = shape_square(p[0]) + shape_square(p[1]);
    const bool in_z = -h2[2] <= p[2] && p[2] < h2[2];
    if (kind == kShapeBox) return -h2[0] <= p[0] && p[0] < h2[0] && -h2[1] <= p[1] && p[1] < h2[1] && in_z;
    if (kind == kShapeBall) return xy + shape_square(p[2]) <= rr;
    if (kind == kShapeCylinder) return xy <= rr && in_z;
    const int64_t q = p[2] < -h2[2] ? -h2[2] : p[2] > h2[2] ? h2[2] : p[2];      // the capsule: the nearest point of its axis
    return xy + shape_square(p[2] - q) <= rr;
}

// Rules 2 and 3: is the cell whose pulled centre is p inside the shape?
VXRT_RULE_FN bool shape_inside(uint32_t kind, int64_t r2, const int64_t* h2, const int64_t* p) {
    return shape_near(p) && shape_holds(kind, r2, h2, p);
}

// Bits 3k of v, k = 0 .. 15, to bits k: spread16's inverse.
VXRT_RULE_FN uint32_t compact16(uint64_t v) {
    uint64_t x = v & 0x249249249249ull;
    x = (x | x >> 2) & 0x0c30c30c30c3ull;
    x = (x | x >> 4) & 0x00f00f00f00full;
    x = (x | x >> 8) & 0x0000ff0000ffull;
    x = (x | x >> 16) & 0xffffull;
    return uint32_t(x);
}

}  // namespace vxrt
