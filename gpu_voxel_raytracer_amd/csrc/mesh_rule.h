// mesh_rule.h — the arithmetic of include/vxrt_mesh.h as the kernels run it (mesh.hip) and as a host compiler reads it
// (tests/test_mesh_cpu.py builds a program of its own around this file): a voxel's coordinates out of its depth-15 path key, the
// face key (direction, plane, the two in-plane coordinates) packed and unpacked, the run-head test between two consecutive sorted
// faces, a quad's four corner keys (linear, so that ascending means (x, y, z)), a corner key as three floats, and the walk to a
// corner's index.  Nothing from HIP is included; the marker is morph_rule.h's, empty for a compiler that is not hipcc.  DESIGN.md §27.
#pragma once
#include <stdint.h>

#include "morph_rule.h"

namespace vxrt {

// vxrt_mesh_mode
constexpr uint32_t kMeshFaces = 0, kMeshRuns = 1;

// Directions are the first six rows of kMorphOffsets: -x, -y, -z, +z, +y, +x.
constexpr uint32_t kMeshDirs = 6;
constexpr uint32_t kMeshDirBits = (uint32_t(1) << kMeshDirs) - 1u;
VXRT_MORPH_FN uint32_t mesh_axis(uint32_t d) { return d < 3u ? d : 5u - d; }
VXRT_MORPH_FN bool mesh_positive(uint32_t d) { return d >= 3u; }

// The faces of a voxel whose 6-neighbour mask is `mask` (bit r: the cell at row r is in the set; a cell outside the range never is).
VXRT_MORPH_FN uint32_t mesh_face_dirs(uint32_t mask) { return ~mask & kMeshDirBits; }

// u = p + 32768 of one axis out of a path key (morph_rule.h: bit k of u at bit 3k + shift; shift 2 is x, 1 is y, 0 is z).
VXRT_MORPH_FN uint32_t mesh_coord(uint64_t key, uint32_t shift) {
    uint64_t v = (key >> shift) & kMorphAxisZ;
    v = (v ^ (v >> 2)) & 0x10c30c30c30c30c3ull;
    v = (v ^ (v >> 4)) & 0x100f00f00f00f00full;
    v = (v ^ (v >> 8)) & 0x001f0000ff0000ffull;
    v = (v ^ (v >> 16)) & 0x001f00000000ffffull;
    v = (v ^ (v >> 32)) & 0xffffull;
    return uint32_t(v);
}

// A face key is (d, w, b, c) compared in that order: 3 + 17 + 16 + 16 = 52 bits.  w is the plane's coordinate on the normal's axis
// a (0 .. 65536: 17 bits), b and c the voxel's coordinates on axes (a + 1) % 3 and (a + 2) % 3, all offset by 32768.
constexpr uint32_t kMeshFaceBits = 52;
VXRT_MORPH_FN uint64_t mesh_face_pack(uint32_t d, uint32_t w, uint32_t b, uint32_t c) {
    return uint64_t(d) << 49 | uint64_t(w) << 32 | uint64_t(b) << 16 | uint64_t(c);
}
struct MeshFace {
    uint32_t d, w, b, c;
};
VXRT_MORPH_FN MeshFace mesh_face_unpack(uint64_t f) {
    return MeshFace{uint32_t(f >> 49) & 7u, uint32_t(f >> 32) & 0x1ffffu, uint32_t(f >> 16) & 0xffffu, uint32_t(f) & 0xffffu};
}

// The face of the voxel of path key `key` in direction d.
VXRT_MORPH_FN uint64_t mesh_face_of(uint64_t key, uint32_t d) {
    const uint32_t x = mesh_coord(key, 2u), y = mesh_coord(key, 1u), z = mesh_coord(key, 0u);
    const uint32_t a = mesh_axis(d);
    const uint32_t ua = a == 0u ? x : a == 1u ? y : z, ub = a == 0u ? y : a == 1u ? z : x, uc = a == 0u ? z : a == 1u ? x : y;
    return mesh_face_pack(d, ua + (mesh_positive(d) ? 1u : 0u), ub, uc);
}

// Rule 3: does the face `cur` begin a quad, `prev` being its predecessor in ascending key order (first: there is none)?  In FACES
// mode every face does.  In RUNS mode it joins prev's quad iff d, w and b agree and c is prev's c + 1 — the keys differ by one and
// prev's c is not 65535, where + 1 would carry into b — and, in a call with bytes (with_words), the two leaf words agree.
VXRT_MORPH_FN bool mesh_is_head(uint64_t prev, uint32_t prev_word, uint64_t cur, uint32_t cur_word, bool first, uint32_t mode, bool with_words) {
    const bool next_cell = (cur == prev + 1u) & ((prev & 0xffffu) != 0xffffu);
    const bool same_bytes = !with_words | (prev_word == cur_word);
    return first | (mode != kMeshRuns) | !(next_cell & same_bytes);
}

// A corner key is x << 34 | y << 17 | z, each of 0 .. 65536: 51 bits, ascending by (x, y, z).
constexpr uint32_t kMeshCornerBits = 51;
VXRT_MORPH_FN uint64_t mesh_corner_pack(uint32_t x, uint32_t y, uint32_t z) { return uint64_t(x) << 34 | uint64_t(y) << 17 | uint64_t(z); }

// Rule 4: the four corners of the quad that begins at face `f` and is `len` faces long, counter-clockwise seen from outside.
struct MeshCorners {
    uint64_t k[4];
};
VXRT_MORPH_FN MeshCorners mesh_quad_corners(uint64_t f, uint32_t len) {
    const MeshFace q = mesh_face_unpack(f);
    const uint32_t a = mesh_axis(q.d), ib = (a + 1u) % 3u, ic = (a + 2u) % 3u;
    const uint32_t b0 = q.b, b1 = q.b + 1u, c0 = q.c, c1 = q.c + len;
    const bool up = mesh_positive(q.d);
    // s > 0: (b0,c0) (b1,c0) (b1,c1) (b0,c1); s < 0: (b0,c0) (b0,c1) (b1,c1) (b1,c0)
    const uint32_t bs[4] = {b0, up ? b1 : b0, b1, up ? b0 : b1};
    const uint32_t cs[4] = {c0, up ? c0 : c1, c1, up ? c1 : c0};
    MeshCorners out;
    for (uint32_t i = 0; i < 4u; i++) {      // selects, not an array indexed by the axis: the kernels keep this in registers
        const uint32_t x = a == 0u ? q.w : ib == 0u ? bs[i] : cs[i];
        const uint32_t y = a == 1u ? q.w : ib == 1u ? bs[i] : cs[i];
        const uint32_t z = a == 2u ? q.w : ib == 2u ? bs[i] : cs[i];
        out.k[i] = mesh_corner_pack(x, y, z);
    }
    (void)ic;
    return out;
}

// Rule 5: a corner as binary32 (integers of magnitude up to 32768 are exact).
struct MeshVertex {
    float v[3];
};
VXRT_MORPH_FN MeshVertex mesh_corner_vertex(uint64_t k) {
    return MeshVertex{{float(int32_t(uint32_t(k >> 34) & 0x1ffffu) - 32768), float(int32_t(uint32_t(k >> 17) & 0x1ffffu) - 32768),
                       float(int32_t(uint32_t(k) & 0x1ffffu) - 32768)}};
}

// The index of q among keys[0 .. m) (ascending, unique, m > 0, q among them): list_has's walk (morph_rule.h) to the greatest index
// whose key is <= q, every load unconditional from a clamped index.
VXRT_MORPH_FN uint32_t mesh_corner_index(const uint64_t* keys, uint32_t m, uint32_t steps, uint64_t q) {
    uint32_t at = 0;
    for (uint32_t s = steps; s != 0u; s--) {
        const uint64_t step = uint64_t(1) << (s - 1u), probe = walk_probe(at, step);
        at = walk_take(keys[list_index(probe, m)], q, at, step, list_there(probe, m));
    }
    return at;
}

}  // namespace vxrt
