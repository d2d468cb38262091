"""CPU: the transform's interface (include/vxrt_transform.h) — plain C, declared once, exported with C linkage by both libraries,
refused without a context — the Python wrappers' signatures and argument checks, which run before any library call; the rule's model
(transform_model.py) against what the rule must give (identity, translations, the 24 axis rotations and their inverses, the two
scales, the ends of the int16 range); rigid_pull and rigid_box; and the kernel's own arithmetic (csrc/transform_rule.h), compiled
by g++ with the undefined-behaviour and address sanitizers into a program of its own, against the model at every limit."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import ray_families as R
import transform_model as T
from conftest import ROOT
from test_components_cpu import bare_context, declared

FUNCTIONS = ["vxrt_transform_voxels_device"]
HEADER = "vxrt_transform.h"
NEW_SOURCES = ("transform.hip", "api_transform.hip", "transform.h", "transform_rule.h")
CSRC = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")


# ---- the header, the libraries, the wrappers ---------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry_point():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt.h"' in text and "typedef struct vxrt_affine" in text
    assert ">> 17" in text and "never wrapped" in text and "rint" in text
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    assert "api_transform.hip" in open(os.path.join(CSRC, "ctx.h")).read()


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), hdr],
                         capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'typedef char affine_is_64[sizeof(vxrt_affine) == 64 ? 1 : -1];\n'
                   'int main(void) {\n'
                   '    size_t n = 7;\n'
                   '    vxrt_affine a = {{{65536, 0, 0}, {0, 65536, 0}, {0, 0, 65536}}, 0, {0, 0, 0}};\n'
                   '    const int32_t lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};\n'
                   '    int rc = vxrt_transform_voxels_device(0, 0, 0, 0, &a, lo, hi, 0, 0, 0, &n);\n'
                   '    return rc == VXRT_E_INVALID && n == 7 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "vxrt.hpp"\nstatic_assert(sizeof(vxrt_affine) == 64, "vxrt_affine");\n'
                   'size_t f(vxrt::Context& c, const int16_t (*p)[3], const uint8_t (*m)[4], const vxrt_affine& a, int16_t (*q)[3], uint8_t (*w)[4]) {\n'
                   '    return c.transform_voxels_device(p, m, 1, a, {0, 0, 0}, {1, 1, 1}) + c.transform_voxels_device(p, m, 1, a, {0, 0, 0}, {1, 1, 1}, q, w, 1); }\n')
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
    out_pos = np.full((2, 3), 0x5A5A, np.uint16)
    out_mrgb = np.full((2, 4), 0xA5, np.uint8)
    pull = H.rigid_pull(np.eye(3))
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(1, 1, 1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = C.c_size_t(7)
    for count in (2, 0, 1 << 32):
        k = C.c_size_t(count)
        assert L.vxrt_transform_voxels_device(None, p(pos), p(mrgb), k, C.byref(pull), lo, hi, p(out_pos), p(out_mrgb), C.c_size_t(2), C.byref(n)) == H.E_INVALID
        assert L.vxrt_transform_voxels_device(None, p(pos), None, k, C.byref(pull), lo, hi, None, None, C.c_size_t(0), C.byref(n)) == H.E_INVALID
        assert L.vxrt_transform_voxels_device(None, None, None, k, None, None, None, None, None, C.c_size_t(0), None) == H.E_INVALID
    assert b"null context" in L.vxrt_last_error()
    assert n.value == 7 and (out_pos == 0x5A5A).all() and (out_mrgb == 0xA5).all() and not pos.any() and (mrgb == 9).all()


def test_the_new_sources_are_built_into_both_libraries():
    from gpu_voxel_raytracer_amd import _build
    for f in NEW_SOURCES:
        assert os.path.exists(os.path.join(CSRC, f)), f
    assert "transform.hip" in _build.SOURCES and "api_transform.hip" in _build.SOURCES      # the variants build takes SOURCES too
    assert "transform.h" in _build.HEADERS and "transform_rule.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)
    rule = open(os.path.join(CSRC, "transform_rule.h")).read()
    assert "#include <hip" not in rule and '#include "' not in rule           # nothing from HIP, nothing of the project's


def test_the_wrapper_signatures(H):
    assert list(inspect.signature(H.Context.transform_voxels).parameters) == ["self", "pos", "mrgb", "pull", "box_min", "box_max", "cap"]
    assert inspect.signature(H.Context.transform_voxels).parameters["cap"].default is None
    assert list(inspect.signature(H.Context.rotate_voxels).parameters) == ["self", "pos", "mrgb", "rotation", "pivot", "translation"]
    assert list(inspect.signature(H.rigid_pull).parameters) == ["rotation", "pivot", "translation"]
    assert list(inspect.signature(H.rigid_box).parameters) == ["src_min", "src_max", "rotation", "pivot", "translation"]
    for f in (H.rigid_pull, H.rigid_box, H.Context.rotate_voxels):
        assert inspect.signature(f).parameters["pivot"].default == (0, 0, 0) and inspect.signature(f).parameters["translation"].default == (0, 0, 0)
    assert C.sizeof(H.Affine) == 64 and C.alignment(H.Affine) == 8 and H.Affine.t.offset == 40 and H.Affine.reserved.offset == 36


def test_the_wrappers_check_their_arguments_before_any_library_call(H):
    import torch
    ctx = bare_context(H)
    try:
        pos, mrgb = np.zeros((5, 3), np.int16), np.zeros((5, 4), np.uint8)
        pull = H.rigid_pull(np.eye(3))
        lo, hi = (0, 0, 0), (4, 4, 4)
        for bad in (pos.astype(np.int32), pos.astype(np.uint16), pos.astype(np.float32), torch.zeros((5, 3), dtype=torch.int32),
                    np.zeros(15, np.int16), np.zeros((5, 4), np.int16), torch.zeros((5, 3), dtype=torch.int16), torch.zeros((3, 5), dtype=torch.int16).t()):
            with pytest.raises(ValueError):
                ctx.transform_voxels(bad, None, pull, lo, hi)
            with pytest.raises(ValueError):
                ctx.rotate_voxels(bad, None, np.eye(3))
        for bad in (mrgb.astype(np.int8), mrgb.astype(np.uint32), np.zeros((5, 3), np.uint8), np.zeros(20, np.uint8), np.zeros((4, 4), np.uint8),
                    torch.zeros((5, 4), dtype=torch.uint8), torch.zeros((4, 5), dtype=torch.uint8).t()):
            with pytest.raises(ValueError):
                ctx.transform_voxels(pos, bad, pull, lo, hi)
            with pytest.raises(ValueError):
                ctx.rotate_voxels(pos, bad, np.eye(3))                     # ... before pos is uploaded
        for bad in (pos.tolist(), None, "pos"):
            with pytest.raises(TypeError):
                ctx.transform_voxels(bad, None, pull, lo, hi)
        with pytest.raises(TypeError):
            ctx.transform_voxels(pos, mrgb.tolist(), pull, lo, hi)
        for bad in (None, np.eye(3), [[65536, 0, 0], [0, 65536, 0], [0, 0, 65536]], "pull"):
            with pytest.raises(TypeError):
                ctx.transform_voxels(pos, mrgb, bad, lo, hi)
        for bad in ((0, 0), (0, 0, 0, 0), (0.5, 0, 0), (32769, 0, 0), (0, -32769, 0), "abc", (None, 0, 0), 3, None):
            with pytest.raises(ValueError):
                ctx.transform_voxels(pos, mrgb, pull, bad, hi)
            with pytest.raises(ValueError):
                ctx.transform_voxels(pos, mrgb, pull, lo, bad)
        for bad in (-1, 1.5, "3", True):
            with pytest.raises(ValueError):
                ctx.transform_voxels(pos, mrgb, pull, lo, hi, cap=bad)
        for bad in (np.eye(4), np.zeros(9), [[1, 0, 0]] * 2, np.full((3, 3), np.nan)):
            with pytest.raises(ValueError):
                ctx.rotate_voxels(pos, None, bad)
            with pytest.raises(ValueError):
                H.rigid_pull(bad)
            with pytest.raises(ValueError):
                H.rigid_box((0, 0, 0), (1, 1, 1), bad)
        for bad in ((0, 0), (np.inf, 0, 0)):
            with pytest.raises(ValueError):
                H.rigid_pull(np.eye(3), bad)
            with pytest.raises(ValueError):
                H.rigid_pull(np.eye(3), (0, 0, 0), bad)
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lists():
    cube = R.scene_voxels("cube16")
    return {"cube16": cube, "shell": T.shell(), "random": T.random_cells()}


def by_path(pos, mrgb):
    """A list deduplicated keep-last and sorted by path key: what the identity returns."""
    src = T.source_of(pos, mrgb)
    keys = sorted(src, key=T.path_key)
    return np.array(keys, np.int16).reshape(-1, 3), np.array([src[k] for k in keys], np.uint8).reshape(-1, 4)


def box_of(pos, grow=0):
    p = np.asarray(pos, np.int64)
    return tuple(int(v) - grow for v in p.min(0)), tuple(int(v) + 1 + grow for v in p.max(0))


def test_identity_is_the_deduplicated_list_in_path_order(lists):
    rng = np.random.default_rng(1)
    cells = rng.integers(-32768, 32768, (1000, 3))
    m, t = T.identity()
    assert all(T.pull_cell(m, t, d) == tuple(d) for d in cells.tolist())
    for name, (pos, mrgb) in lists.items():
        want_pos, want_mrgb = by_path(pos, mrgb)
        got_pos, got_mrgb = T.transform(pos, mrgb, m, t, *box_of(pos, 1))
        assert np.array_equal(got_pos, want_pos) and np.array_equal(got_mrgb, want_mrgb), name
        assert (got_mrgb[:, 0] < 0x80).all()
        only_pos, none = T.transform(pos, None, m, t, *box_of(pos, 1))
        assert none is None and np.array_equal(only_pos, want_pos)
    pos, mrgb = lists["random"]
    assert len(by_path(pos, mrgb)[0]) < len(pos)                      # it has duplicates, and the last entry's bytes win
    twice = np.array([[1, 2, 3]] * 4, np.int16)
    colours = np.array([[0x81, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [0xFF, 4, 5, 6]], np.uint8)
    got = T.transform(twice, colours, m, t, (0, 0, 0), (4, 4, 4))
    assert got[0].tolist() == [[1, 2, 3]] and got[1].tolist() == [[0x7F, 4, 5, 6]]


def test_an_integer_translation_is_pos_plus_offset(lists):
    pos, mrgb = lists["cube16"]
    base_pos, base_mrgb = by_path(pos, mrgb)
    for offset in ((1, 0, 0), (-9, 4, 17), (0, 0, -8), (-3, -3, -3)):
        m, t = T.translation(offset)
        moved = pos.astype(np.int64) + np.array(offset)
        got_pos, got_mrgb = T.transform(pos, mrgb, m, t, *box_of(moved, 2))
        want_pos, want_mrgb = by_path(moved, mrgb)
        assert np.array_equal(got_pos, want_pos) and np.array_equal(got_mrgb, want_mrgb), offset
        assert len(got_pos) == len(base_pos)


@pytest.mark.parametrize("twice_pivot", [(0, 0, 0), (1, 1, 1), (5, -3, 7)])
def test_each_axis_rotation_is_a_bijection_and_its_inverse_returns_the_list(lists, twice_pivot):
    pos, mrgb = lists["shell"]
    want_pos, want_mrgb = by_path(pos, mrgb)
    big = (-18, -18, -18), (18, 18, 18)      # the shell spans [-9, 8]; the farthest pivot is 3.5 from the origin on an axis
    seen = set()
    for r in T.axis_rotations():
        m, t = T.rotation_pull(r, twice_pivot)
        assert all(v in (0, T.ONE, -T.ONE) for row in m for v in row)
        there_pos, there_mrgb = T.transform_np(pos, mrgb, m, t, *big)
        assert len(there_pos) == len(want_pos)                                       # a bijection of the cells
        assert sorted(there_mrgb.tolist()) == sorted(want_mrgb.tolist())
        seen.add(there_pos.tobytes() + there_mrgb.tobytes())
        inverse = [[r[j][i] for j in range(3)] for i in range(3)]
        back_pos, back_mrgb = T.transform_np(there_pos, there_mrgb, *T.rotation_pull(inverse, twice_pivot), *big)
        assert np.array_equal(back_pos, want_pos) and np.array_equal(back_mrgb, want_mrgb), r
    assert len(seen) == 24                                     # the shell is symmetric, its colours are not: 24 different results
    # about the origin the pull is exactly s = (R^T (2d + 1) - 1) / 2
    if twice_pivot == (0, 0, 0):
        for r in T.axis_rotations()[:6]:
            m, t = T.rotation_pull(r)
            for d in ((0, 0, 0), (3, -5, 7), (-32768, 32767, 1)):
                c = [2 * v + 1 for v in d]
                want = tuple((sum(r[j][i] * c[j] for j in range(3)) - 1) // 2 for i in range(3))
                assert T.pull_cell(m, t, d) == want


def test_the_two_scales(lists):
    pos, mrgb = lists["cube16"]
    base_pos, base_mrgb = by_path(pos, mrgb)
    src = T.source_of(pos, mrgb)
    # m = 1/2: every voxel becomes the 2 x 2 x 2 block of cells 2 s .. 2 s + 1
    m, t = T.scale(32768)
    got_pos, got_mrgb = T.transform(pos, mrgb, m, t, (-20, -20, -20), (20, 20, 20))
    assert len(got_pos) == 8 * len(base_pos)
    for d, b in zip(got_pos.tolist(), got_mrgb.tolist()):
        assert src[tuple(v >> 1 for v in d)] == tuple(b)
    # m = 2: cell d takes source cell 2 d + 1: the voxels at odd coordinates stay
    m, t = T.scale(131072)
    got_pos, got_mrgb = T.transform(pos, mrgb, m, t, (-20, -20, -20), (20, 20, 20))
    odd = [p for p in base_pos.tolist() if all(v & 1 for v in p)]
    assert len(got_pos) == len(odd) > 100
    assert sorted(got_pos.tolist()) == sorted([[(v - 1) // 2 for v in p] for p in odd])


def test_the_ends_of_the_int16_range():
    m, t = T.identity()
    pos = np.array([[32767, -32768, 0]], np.int16)
    mrgb = np.array([[1, 2, 3, 4]], np.uint8)
    got = T.transform(pos, mrgb, m, t, (32766, -32768, -1), (32768, -32766, 2))
    assert got[0].tolist() == [[32767, -32768, 0]] and got[1].tolist() == [[1, 2, 3, 4]]         # reachable
    # a pull that lands at 32768 or at -32769 is absent: with wrapped coordinates it would find the voxel at the other end
    ends = np.array([[-32768, 0, 0], [32767, 1, 1]], np.int16)
    m, t = T.translation((-1, 0, 0))                  # s = d + 1
    assert T.pull_cell(m, t, (32767, 0, 0)) == (32768, 0, 0) and not T.in_range((32768, 0, 0))
    assert len(T.transform(ends, None, m, t, (32767, 0, 0), (32768, 1, 1))[0]) == 0
    assert T.transform(ends, None, m, t, (32766, 1, 1), (32768, 2, 2))[0].tolist() == [[32766, 1, 1]]
    m, t = T.translation((1, 0, 0))                   # s = d - 1
    assert T.pull_cell(m, t, (-32768, 1, 1)) == (-32769, 1, 1) and not T.in_range((-32769, 1, 1))
    assert len(T.transform(ends, None, m, t, (-32768, 1, 1), (-32767, 2, 2))[0]) == 0
    assert T.transform(ends, None, m, t, (-32768, 0, 0), (-32766, 1, 1))[0].tolist() == [[-32767, 0, 0]]


def test_path_order_does_not_depend_on_the_depth():
    rng = np.random.default_rng(4)
    pts = rng.integers(-16, 16, (4000, 3)).tolist()
    orders = [sorted(range(len(pts)), key=lambda i: (T.path_key(pts[i], depth), i)) for depth in (4, 9, 15)]
    assert orders[0] == orders[1] == orders[2]


def test_the_numpy_walk_equals_the_model(lists):
    pos, mrgb = lists["random"]
    for k, r in enumerate(T.GENERAL_ROTATIONS):
        from gpu_voxel_raytracer_amd import host as H
        a = H.rigid_pull(r, (20, 20, 20), (k, -k, 3))
        m, t = [list(row) for row in a.m], list(a.t)
        box = (5, 0, 10), (30, 33, 29)
        for colours in (mrgb, None):
            want, got = T.transform(pos, colours, m, t, *box), T.transform_np(pos, colours, m, t, *box)
            assert np.array_equal(want[0], got[0]) and len(want[0]) > 1000
            assert (want[1] is None and got[1] is None) if colours is None else np.array_equal(want[1], got[1])
    assert len(T.transform_np(pos, mrgb, *T.identity(), (0, 0, 0), (0, 5, 5))[0]) == 0
    assert len(T.transform_np(pos[:0], mrgb[:0], *T.identity(), (0, 0, 0), (5, 5, 5))[0]) == 0


# ---- rigid_pull and rigid_box ------------------------------------------------------------------------------------------------------
def test_the_axis_rotations_give_exact_maps(H):
    for r in T.axis_rotations():
        for twice_pivot in ((0, 0, 0), (1, 1, 1), (5, -3, 7)):
            a = H.rigid_pull(np.array(r, np.float64), tuple(v / 2 for v in twice_pivot))
            m, t = T.rotation_pull(r, twice_pivot)
            assert [list(row) for row in a.m] == m and list(a.t) == t and a.reserved == 0
            assert all(v in (0, 65536, -65536) for row in a.m for v in row)
    with pytest.raises(ValueError):
        H.rigid_pull(np.eye(3) * 257.0)                                  # |m| beyond 2^24
    with pytest.raises(ValueError):
        H.rigid_pull(np.eye(3), (0, 0, 0), (2.0 ** 25, 0, 0))             # |t| beyond 2^40
    assert H.rigid_box((-32768, 0, 0), (32767, 0, 0), np.eye(3)) == ((-32768, -2, -2), (32768, 3, 3))     # clipped


def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_rigid_box_holds_every_cell_that_pulls_a_voxel(H, lists):
    rng = np.random.default_rng(23)
    for name, (pos, mrgb) in lists.items():
        lo, hi = pos.min(0).astype(int), pos.max(0).astype(int)
        for trial in range(4):
            r = random_rotation(rng)
            pivot = tuple((rng.integers(-40, 40, 3) + (0.5 if trial % 2 else 0.0)).tolist())
            shift = tuple(rng.integers(-30, 30, 3).tolist()) if trial < 3 else (20000.25, -15000.5, 3.75)
            a = H.rigid_pull(r, pivot, shift)
            m, t = [list(row) for row in a.m], list(a.t)
            box = H.rigid_box(lo, hi, r, pivot, shift)
            inner, _ = T.transform_np(pos, None, m, t, *box)
            wide = tuple(v - 4 for v in box[0]), tuple(v + 4 for v in box[1])
            outer, _ = T.transform_np(pos, None, m, t, *wide)
            assert len(outer) == len(inner) > 0.8 * len(T.source_of(pos)), (name, trial)
            assert np.array_equal(outer, inner), (name, trial)


# ---- the kernel's arithmetic as a host compiler reads it --------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "transform_rule.h"
int main() {
    long long v[15];
    for (;;) {
        for (int k = 0; k < 15; k++)
            if (std::scanf("%lld", &v[k]) != 1) return k == 0 ? 0 : 2;
        int32_t m[3][3], d[3];
        int64_t t[3], s[3];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) m[i][j] = int32_t(v[3 * i + j]);
            t[i] = v[9 + i];
            d[i] = int32_t(v[12 + i]);
        }
        vxrt::pull_cell(m, t, d, s);
        const bool in = vxrt::pull_in_range(s);
        std::printf("%lld %lld %lld %d %llu\n", (long long)s[0], (long long)s[1], (long long)s[2], in ? 1 : 0,
                    (unsigned long long)(in ? vxrt::path_key15(int32_t(s[0]), int32_t(s[1]), int32_t(s[2])) : 0));
    }
}
"""


def build_rule_program(tmp_path):
    """DRIVER around csrc/transform_rule.h under the undefined-behaviour and address sanitizers -> the program's path"""
    src = tmp_path / "rule.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "rule"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                            "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def rule_program_agrees_with_the_model(exe, cases):
    """(m, t, d) triples through the program: its output equals the model's and the sanitizers report nothing -> how many are in range"""
    text = "".join(" ".join(str(int(v)) for row in m for v in row) + " " + " ".join(str(int(v)) for v in t) + " " + " ".join(str(int(v)) for v in d) + "\n"
                   for m, t, d in cases)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-2000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    in_count = 0
    for (m, t, d), line in zip(cases, lines):
        s = T.pull_cell(m, t, d)
        inside = T.in_range(s)
        in_count += inside
        want = f"{s[0]} {s[1]} {s[2]} {1 if inside else 0} {T.path_key(s) if inside else 0}"
        assert line == want, (m, t, d, line, want)
    return in_count


def test_the_kernels_arithmetic_under_the_sanitizers(tmp_path):
    exe = build_rule_program(tmp_path)
    rng = np.random.default_rng(17)
    big_m, big_t = T.M_LIMIT, T.T_LIMIT
    cases = []
    ends = (-32768, -32767, -1, 0, 1, 32766, 32767)
    for sm in (big_m, -big_m):
        for st in (big_t, -big_t, 0):
            for d in ends:
                cases.append(([[sm] * 3] * 3, [st] * 3, [d] * 3))
                cases.append(([[sm, -sm, sm], [-sm, -sm, -sm], [0, sm, 0]], [st, -st, st], [d, -1 - d, d]))
    for d in ends:
        cases.append((T.identity()[0], [0, 0, 0], [d, d, d]))
        cases.append((T.identity()[0], [T.ONE, -T.ONE, 0], [d, d, d]))              # lands at 32768 / -32769 at the ends
        cases.append((T.scale(-T.ONE)[0], [0, 0, 0], [d, -d - 1, 0]))               # negative sums
        cases.append((T.scale(1)[0], [-1, 1, 0], [d, d, d]))                        # the least nonzero entries
    for _ in range(400):
        wide = rng.random() < 0.5
        m = rng.integers(-big_m if wide else -2 * T.ONE, (big_m if wide else 2 * T.ONE) + 1, (3, 3)).tolist()
        t = rng.integers(-big_t if wide else -(T.ONE << 15), (big_t if wide else T.ONE << 15) + 1, 3).tolist()
        cases.append((m, t, rng.integers(-32768, 32768, 3).tolist()))
    in_count = rule_program_agrees_with_the_model(exe, cases)
    assert 50 < in_count < len(cases) - 50                                  # both answers of the range test are exercised
