"""CPU: the mesher's interface (include/vxrt_mesh.h) — plain C, declared once, exported with C linkage by both libraries, refused
without a context — the Python wrapper's signature and argument checks, which run before any library call; the rule's model
(mesh_model.py) against the solid voxeliser's model (solid_model.interior along z and along x: the mesh's inside is the set), against
the signed volume, the edge parity and the faces' count; and the kernels' own arithmetic (csrc/mesh_rule.h: the face key, the head
test, the corner keys, the vertex, the index walk), compiled by g++ with the undefined-behaviour and address sanitizers into a
program of its own that takes sorted keys and words as the kernels do, against the model bit for bit."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import mesh_model as MM
import morph_model as M
import solid_model as S
from conftest import ROOT
from test_components_cpu import bare_context, declared
from transform_model import source_of

FUNCTIONS = ["vxrt_mesh_voxels_device"]
HEADER = "vxrt_mesh.h"
NEW_SOURCES = ("mesh.hip", "api_mesh.hip", "mesh.h", "mesh_rule.h")
CSRC = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")


# ---- the header, the libraries, the wrapper ----------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry_point():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt.h"' in text and "typedef enum vxrt_mesh_mode" in text
    for phrase in ("last entry of a position wins", "counter-clockwise seen from outside", "T-junctions", "even number of triangles",
                   "12 triangles and 8 vertices", "32767", "ascending by (x, y, z)"):
        assert phrase in text, phrase
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    assert "api_mesh.hip" in open(os.path.join(CSRC, "ctx.h")).read()
    assert len(declared("vxrt.h")) <= 40


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), hdr],
                         capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'typedef char modes_are_0_and_1[VXRT_MESH_FACES == 0 && VXRT_MESH_RUNS == 1 ? 1 : -1];\n'
                   'int main(void) {\n'
                   '    size_t v = 7, t = 9;\n'
                   '    vxrt_mesh_mode mode = VXRT_MESH_RUNS;\n'
                   '    int rc = vxrt_mesh_voxels_device(0, 0, 0, 0, (uint32_t)mode, 0, 0, 0, 0, 0, &v, &t);\n'
                   '    return rc == VXRT_E_INVALID && v == 7 && t == 9 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "vxrt.hpp"\n'
                   'size_t f(vxrt::Context& c, const int16_t (*p)[3], const uint8_t (*m)[4], float (*v)[3], uint32_t (*t)[3], uint8_t (*w)[4]) {\n'
                   '    return c.mesh_voxels_device(p, nullptr, 1).first + c.mesh_voxels_device(p, m, 1, VXRT_MESH_FACES, v, 8, t, w, 12).second; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cpp)], check=True)


def test_both_libraries_export_it_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    for lib in (_build.LIB, H.variants_library()):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
        for f in FUNCTIONS:
            assert f in exported, (lib, f)          # unmangled => extern "C"
    assert H.lib().vxrt_abi_version() == 6


def test_a_null_context_is_invalid(H):
    L = H.lib()
    pos = np.zeros((2, 3), np.int16)
    mrgb = np.full((2, 4), 9, np.uint8)
    verts = np.full((64, 3), 7.5, np.float32)
    tris = np.full((64, 3), 0x5A5A5A5A, np.uint32)
    out_mrgb = np.full((64, 4), 0xA5, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    v, t = C.c_size_t(7), C.c_size_t(9)
    for count in (2, 0, 1 << 32):
        k = C.c_size_t(count)
        for mode in (0, 1, 2):
            assert L.vxrt_mesh_voxels_device(None, p(pos), p(mrgb), k, C.c_uint32(mode), p(verts), C.c_size_t(64), p(tris), p(out_mrgb),
                                             C.c_size_t(64), C.byref(v), C.byref(t)) == H.E_INVALID
            assert L.vxrt_mesh_voxels_device(None, p(pos), None, k, C.c_uint32(mode), None, C.c_size_t(0), None, None, C.c_size_t(0),
                                             C.byref(v), C.byref(t)) == H.E_INVALID
            assert L.vxrt_mesh_voxels_device(None, None, None, k, C.c_uint32(mode), None, C.c_size_t(0), None, None, C.c_size_t(0), None, None) == H.E_INVALID
    assert b"null context" in L.vxrt_last_error()
    assert (v.value, t.value) == (7, 9) and (verts == 7.5).all() and (tris == 0x5A5A5A5A).all() and (out_mrgb == 0xA5).all()
    assert not pos.any() and (mrgb == 9).all()


def test_the_new_sources_are_built_into_both_libraries():
    from gpu_voxel_raytracer_amd import _build
    for f in NEW_SOURCES:
        assert os.path.exists(os.path.join(CSRC, f)), f
    assert "mesh.hip" in _build.SOURCES and "api_mesh.hip" in _build.SOURCES      # the variants build takes SOURCES too
    assert "mesh.h" in _build.HEADERS and "mesh_rule.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)
    rule = open(os.path.join(CSRC, "mesh_rule.h")).read()
    assert "#include <hip" not in rule and rule.count('#include "') == 1 and '#include "morph_rule.h"' in rule      # nothing from HIP


def test_the_wrapper_signature_and_constants(H):
    params = inspect.signature(H.Context.mesh_voxels).parameters
    assert list(params) == ["self", "pos", "mrgb", "mode", "cap"]
    assert (params["mode"].default, params["cap"].default) == (H.MESH_RUNS, None)
    assert (H.MESH_FACES, H.MESH_RUNS) == (0, 1) == MM.MODES


def test_the_wrapper_checks_its_arguments_before_any_library_call(H):
    import torch
    ctx = bare_context(H)
    try:
        pos, mrgb = np.zeros((5, 3), np.int16), np.zeros((5, 4), np.uint8)
        for bad in (pos.astype(np.int32), pos.astype(np.uint16), pos.astype(np.float32), torch.zeros((5, 3), dtype=torch.int32), np.zeros(15, np.int16),
                    np.zeros((5, 4), np.int16), torch.zeros((5, 3), dtype=torch.int16), torch.zeros((3, 5), dtype=torch.int16).t()):
            with pytest.raises(ValueError):
                ctx.mesh_voxels(bad, None)
        for bad in (mrgb.astype(np.int8), mrgb.astype(np.uint32), np.zeros((5, 3), np.uint8), np.zeros(20, np.uint8), np.zeros((4, 4), np.uint8),
                    torch.zeros((5, 4), dtype=torch.uint8), torch.zeros((4, 5), dtype=torch.uint8).t()):
            with pytest.raises(ValueError):
                ctx.mesh_voxels(pos, bad)                                  # ... before anything is uploaded
        for bad in (pos.tolist(), None, "pos"):
            with pytest.raises(TypeError):
                ctx.mesh_voxels(bad, None)
        with pytest.raises(TypeError):
            ctx.mesh_voxels(pos, mrgb.tolist())
        for bad in (-1, 2, 1.0, "1", None, True):
            with pytest.raises(ValueError):
                ctx.mesh_voxels(pos, mrgb, bad)
        for bad in (5, -1, (5,), (5, 5, 5), (5, -1), (1.5, 5), ("3", 5), (True, 5), (None, 5), "ab"):
            with pytest.raises(ValueError):
                ctx.mesh_voxels(pos, mrgb, H.MESH_FACES, cap=bad)
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


# ---- the model -------------------------------------------------------------------------------------------------------------------
def cells_of(pos):
    return {tuple(p) for p in np.asarray(pos).tolist()}


def colourings(n, seed):
    return (("positions only", None), ("one colour", MM.one_colour(n)), ("three colours", MM.three_colours(n, seed)))


def test_one_voxel_by_hand():
    verts, tris, mrgb = MM.mesh(MM.cells((3, -4, 5)), np.array([[0x85, 1, 2, 3]], np.uint8), MM.RUNS)
    assert verts.tolist() == [[x, y, z] for x in (3, 4) for y in (-4, -3) for z in (5, 6)]
    assert len(tris) == 12 and set(map(tuple, mrgb.tolist())) == {(5, 1, 2, 3)}
    # the first quad is the -x face at x = 3: (y, z) = (-4, 5), (-4, 6), (-3, 6), (-3, 5), seen from -x counter-clockwise
    assert [verts[i].tolist() for i in tris[0]] == [[3, -4, 5], [3, -4, 6], [3, -3, 6]]
    assert [verts[i].tolist() for i in tris[1]] == [[3, -4, 5], [3, -3, 6], [3, -3, 5]]
    # the last is the +x face at x = 4: (-4, 5), (-3, 5), (-3, 6), (-4, 6)
    assert [verts[i].tolist() for i in tris[10]] == [[4, -4, 5], [4, -3, 5], [4, -3, 6]]
    assert MM.volume6(verts, tris) == 6


def test_runs_by_hand():
    # 1 x 1 x 4 along z: the x-normal faces run along z (one quad each), the y-normal faces run along x and the z-normal ones along
    # y (one cell each): 2 + 8 + 2 quads
    column = MM.block((0, 0, 0), (1, 1, 4))
    assert sorted(MM.quad_areas(column, None, MM.RUNS)) == [1] * 10 + [4, 4]
    assert MM.quad_areas(column, None, MM.FACES) == [1] * 18
    # two colours, changing at z = 2: the long quads break there
    two = np.array([[1, 9, 9, 9]] * 2 + [[2, 9, 9, 9]] * 2, np.uint8)
    assert sorted(MM.quad_areas(column, two, MM.RUNS)) == [1] * 10 + [2] * 4
    # bit 7 of the material byte never matters: it does not break a run
    assert sorted(MM.quad_areas(column, np.array([[1, 9, 9, 9], [0x81, 9, 9, 9]] * 2, np.uint8), MM.RUNS)) == [1] * 10 + [4, 4]
    # a run does not go on from z = 32767 of one row to z = -32768 of the next
    ends = MM.cells((0, 0, 32767), (0, 1, -32768))
    assert MM.quad_areas(ends, None, MM.RUNS) == [1] * 12
    # T-junctions in RUNS mode: some edge has an odd number of triangles; none in FACES mode
    ell = MM.cells((0, 0, 0), (0, 0, 1), (0, 1, 0))
    assert any(c % 2 for c in MM.edge_counts(MM.mesh(ell, None, MM.RUNS)[1]).values())
    assert not any(c % 2 for c in MM.edge_counts(MM.mesh(ell, None, MM.FACES)[1]).values())


@pytest.mark.parametrize("name,pos", MM.small_families(), ids=[n for n, _ in MM.small_families()])
def test_the_inside_of_the_mesh_is_the_set(name, pos):
    want = sorted(cells_of(pos))
    for what, mrgb in colourings(len(pos), 3):
        faces = MM.mesh(pos, mrgb, MM.FACES)
        for mode in MM.MODES:
            verts, tris, out = MM.mesh(pos, mrgb, mode)
            assert (out is None) == (mrgb is None) and (out is None or len(out) == len(tris))
            assert len(np.unique(tris)) == len(verts)                                   # no vertex is unused
            assert [tuple(v) for v in verts.tolist()] == sorted(set(map(tuple, verts.tolist())))
            for axis in (2, 0):
                got = S.interior(verts, tris, axis=axis)
                assert sorted(map(tuple, got.tolist())) == want, (name, what, MM.NAMES[mode], axis)
            assert MM.volume6(verts, tris) == 6 * len(want), (name, what, MM.NAMES[mode])
            assert sum(MM.quad_areas(pos, mrgb, mode)) == len(faces[1]) // 2
        assert not any(c % 2 for c in MM.edge_counts(faces[1]).values()), (name, what)
        assert len(faces[1]) <= 12 * len(pos) and len(faces[0]) <= 8 * len(pos)
        if mrgb is not None:                                                            # each triangle carries its voxel's bytes
            src = source_of(pos, mrgb)
            verts, tris, out = faces
            for t, b in zip(tris.tolist(), out.tolist()):
                tri = verts[t]
                normal = np.cross(tri[1] - tri[0], tri[2] - tri[0])
                voxel = np.floor(tri.mean(axis=0) - normal / np.abs(normal).sum() * 0.5).astype(int)
                assert src[tuple(voxel.tolist())] == tuple(b)


# ---- the kernels' arithmetic ---------------------------------------------------------------------------------------------------
DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "mesh_rule.h"

using namespace vxrt;

// pack and unpack, the coordinates of a key and the corner keys at the ends of every field
static int fields() {
    const uint32_t ws[] = {0u, 1u, 32768u, 65535u, 65536u}, cs[] = {0u, 1u, 32767u, 32768u, 65534u, 65535u};
    for (uint32_t d = 0; d < kMeshDirs; d++)
        for (uint32_t w : ws)
            for (uint32_t b : cs)
                for (uint32_t c : cs) {
                    const uint64_t f = mesh_face_pack(d, w, b, c);
                    const MeshFace u = mesh_face_unpack(f);
                    if (u.d != d || u.w != w || u.b != b || u.c != c || (f >> kMeshFaceBits) != 0u) return 30;
                    if (d + 1u < kMeshDirs && !(f < mesh_face_pack(d + 1u, 0u, 0u, 0u))) return 31;
                    if (w != 65536u && !(f < mesh_face_pack(d, w + 1u, 0u, 0u))) return 32;
                    const uint64_t k = mesh_corner_pack(w, b + 1u, c + 1u);
                    if ((k >> kMeshCornerBits) != 0u) return 33;
                    const MeshVertex v = mesh_corner_vertex(k);
                    if (v.v[0] != float(int(w) - 32768) || v.v[1] != float(int(b) - 32767) || v.v[2] != float(int(c) - 32767)) return 34;
                }
    if (mesh_axis(0) != 0 || mesh_axis(1) != 1 || mesh_axis(2) != 2 || mesh_axis(3) != 2 || mesh_axis(4) != 1 || mesh_axis(5) != 0) return 35;
    for (uint32_t d = 0; d < kMeshDirs; d++)
        if (kMorphOffsets[d].d[mesh_axis(d)] != (mesh_positive(d) ? 1 : -1)) return 36;
    // the head test: a face one cell on joins, unless the cell before is the row's last, the bytes differ, or the mode is FACES
    const uint64_t f = mesh_face_pack(5, 40000, 7, 100);
    if (mesh_is_head(f, 1, f + 1, 1, false, kMeshRuns, true)) return 40;
    if (!mesh_is_head(f, 1, f + 1, 2, false, kMeshRuns, true)) return 41;
    if (mesh_is_head(f, 1, f + 1, 2, false, kMeshRuns, false)) return 42;
    if (!mesh_is_head(f, 1, f + 1, 1, false, kMeshFaces, true)) return 43;
    if (!mesh_is_head(f, 1, f + 1, 1, true, kMeshRuns, true)) return 44;
    if (!mesh_is_head(f, 1, f + 2, 1, false, kMeshRuns, true)) return 45;
    if (!mesh_is_head(mesh_face_pack(5, 40000, 7, 65535), 1, mesh_face_pack(5, 40000, 8, 0), 1, false, kMeshRuns, true)) return 46;
    if (mesh_is_head(mesh_face_pack(5, 40000, 7, 65534), 1, mesh_face_pack(5, 40000, 7, 65535), 1, false, kMeshRuns, true)) return 47;
    if (!mesh_is_head(mesh_face_pack(4, 65536, 65535, 65535), 1, mesh_face_pack(5, 0, 0, 0), 1, false, kMeshRuns, true)) return 48;
    return 0;
}

int main() {
    if (int rc = fields()) return rc;
    unsigned mode, with_words, m;
    while (std::scanf("%u %u %u", &mode, &with_words, &m) == 3) {
        std::vector<uint64_t> keys(m ? m : 2);
        std::vector<uint32_t> words(m ? m : 2);
        for (unsigned i = 0; i < m; i++) {
            unsigned long long k;
            unsigned w;
            if (std::scanf("%llu %u", &k, &w) != 2) return 2;
            keys[i] = k;
            words[i] = w;
        }
        // the masks, as morph.hip gives them at connectivity 6, and the faces in the emit kernel's order
        const uint32_t steps = list_steps(m);
        std::vector<std::pair<uint64_t, uint32_t>> faces;
        for (uint32_t i = 0; i < m; i++) {
            uint32_t mask = 0;
            for (uint32_t r = 0; r < kMeshDirs; r++) {
                bool ok;
                const uint64_t q = neighbour_key(keys[i], r, &ok);
                mask |= (list_has(keys.data(), m, steps, q, ok) ? 1u : 0u) << r;
            }
            for (uint32_t d = 0; d < kMeshDirs; d++)
                if (mesh_face_dirs(mask) >> d & 1u) faces.push_back({mesh_face_of(keys[i], d), words[i]});
        }
        std::sort(faces.begin(), faces.end());
        const uint32_t count = uint32_t(faces.size());
        std::vector<uint32_t> heads;
        for (uint32_t i = 0; i < count; i++) {
            const uint32_t before = morph_safe_index(i - 1u, count);      // wraps at 0, as in the kernel
            if (i != 0 && faces[i].first == faces[before].first) return 3;      // a face key names one face
            if (mesh_is_head(faces[before].first, faces[before].second, faces[i].first, faces[i].second, i == 0u, mode, with_words != 0u)) heads.push_back(i);
        }
        const uint32_t quads = uint32_t(heads.size());
        std::vector<uint64_t> corners;
        for (uint32_t j = 0; j < quads; j++) {
            const uint32_t end = j + 1u < quads ? heads[j + 1u] : count;
            const MeshCorners c = mesh_quad_corners(faces[heads[j]].first, end - heads[j]);
            corners.insert(corners.end(), c.k, c.k + 4);
        }
        std::vector<uint64_t> verts(corners);
        std::sort(verts.begin(), verts.end());
        verts.erase(std::unique(verts.begin(), verts.end()), verts.end());
        const uint32_t n_verts = uint32_t(verts.size()), vsteps = list_steps(n_verts);
        if (verts.empty()) verts.resize(2);
        std::printf("mesh %u %u\n", n_verts, 2u * quads);
        for (uint32_t i = 0; i < n_verts; i++) {
            const MeshVertex v = mesh_corner_vertex(verts[i]);
            std::printf("%.1f %.1f %.1f\n", double(v.v[0]), double(v.v[1]), double(v.v[2]));
        }
        for (uint32_t j = 0; j < quads; j++) {
            uint32_t at[4];
            for (uint32_t i = 0; i < 4u; i++) {
                at[i] = mesh_corner_index(verts.data(), n_verts, vsteps, corners[4u * j + i]);
                if (verts[at[i]] != corners[4u * j + i]) return 4;
            }
            std::printf("%u %u %u %u\n%u %u %u %u\n", at[0], at[1], at[2], faces[heads[j]].second, at[0], at[2], at[3], faces[heads[j]].second);
        }
    }
    return 0;
}
"""


def key_cases():
    """[(name, pos, mrgb or None)]"""
    rng = np.random.default_rng(31)
    cases = []
    for name, pos in MM.small_families():
        for what, mrgb in colourings(len(pos), 5):
            cases.append((f"{name}, {what}", pos, mrgb))
    cases.append(("nothing", np.zeros((0, 3), np.int16), None))
    corners = np.array([[x, y, z] for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)], np.int16)
    cases.append(("the range's corners", corners, MM.three_colours(8, 6)))
    for axis in range(3):
        for at in (-32768, 32766):
            pair = np.zeros((2, 3), np.int16)
            pair[:, axis] = (at, at + 1)
            cases.append((f"a pair at {at} on axis {axis}", pair, MM.one_colour(2)))
    cases.append(("one row's end and the next row's start", MM.cells((0, 0, 32767), (0, 1, -32768), (32767, 5, 0), (-32768, 5, 1)), None))
    cases.append(("a bar along z", MM.bar(2, 300, -150), MM.three_colours(300, 7)))
    cases.append(("a bar along x", MM.bar(0, 300, 32468), None))
    for _ in range(40):
        side = int(rng.choice([3, 5, 9]))
        origin = np.array([int(rng.choice([-32768, -side // 2, 32768 - side])) for _ in range(3)])
        n = int(rng.integers(1, 200))
        pos = (rng.integers(0, side, (n, 3)) + origin).astype(np.int16)
        cases.append(("random", pos, None if rng.random() < 0.3 else MM.three_colours(n, int(rng.integers(100)))))
    # keys whose coordinates differ in bits 6 to 14, and patches on every face, edge and corner of the range (list_families.py)
    import list_families as LF
    for case in (LF.seams()[0], LF.range_faces()[0]):
        cases.append((case.name, case.pos, case.mrgb))
    return cases


def run_rule_program(exe, runs):
    """runs: [(mode, with words, keys, words)] through the program (test_morph_cpu.build_rule_program of DRIVER) ->
    [(verts float32 [V,3], rows int64 [T,4]: a triangle's three indices and its quad's leaf word)] per run, each held to the counts
    the program prints in front of it."""
    text = "".join(f"{mode} {1 if with_words else 0} {len(keys)}\n" + "".join(f"{k} {w}\n" for k, w in zip(keys, words)) for mode, with_words, keys, words in runs)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (run.returncode, run.stderr[-2000:])
    lines = iter(run.stdout.split("\n"))
    results = []
    for n in range(len(runs)):
        head = next(lines).split()
        assert len(head) == 3 and head[0] == "mesh", (n, head)
        n_verts, n_tris = int(head[1]), int(head[2])
        verts = np.array([next(lines).split() for _ in range(n_verts)], np.float64).reshape(-1, 3).astype(np.float32)
        rows = np.array([next(lines).split() for _ in range(n_tris)], np.int64).reshape(-1, 4)
        results.append((verts, rows))
    assert next(lines) == ""
    return results


def test_the_kernels_arithmetic_under_the_sanitizers(tmp_path):
    from test_morph_cpu import build_rule_program
    exe = build_rule_program(tmp_path, DRIVER)
    runs = []
    for name, pos, mrgb in key_cases():
        keys, words = M.sorted_keys_words(pos, mrgb)
        for mode in MM.MODES:
            runs.append((name, pos, mrgb, mode, keys, words))
    merged = 0
    results = run_rule_program(exe, [(mode, mrgb is not None, keys, words) for _, _, mrgb, mode, keys, words in runs])
    for (name, pos, mrgb, mode, _, _), (got, rows) in zip(runs, results):
        verts, tris, out = MM.mesh(pos, mrgb, mode)
        assert (len(got), len(rows)) == (len(verts), len(tris)), (name, MM.NAMES[mode])
        assert got.tobytes() == verts.tobytes(), (name, MM.NAMES[mode])
        assert np.array_equal(rows[:, :3], tris), (name, MM.NAMES[mode])
        if mrgb is not None:
            assert [M.word_bytes(int(w)) for w in rows[:, 3]] == [tuple(b) for b in out.tolist()], (name, MM.NAMES[mode])
        merged += mode == MM.RUNS and len(tris) < len(MM.mesh(pos, mrgb, MM.FACES)[1])
    assert merged > 10
