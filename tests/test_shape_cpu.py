"""CPU: the shape rasteriser's interface (include/vxrt_shape.h) — plain C, declared once, exported with C linkage by both libraries,
refused without a context — the Python wrappers' signatures and argument checks, which run before any library call; the rule's model
(shape_model.py) against what the rule must give (counts known by hand, the cube's symmetries, boxes that tile, inclusions between
the kinds); the host helpers' boxes; and the kernel's own arithmetic (csrc/shape_rule.h), compiled by g++ with the
undefined-behaviour and address sanitizers into a program of its own, against the model at every limit."""
import ctypes as C
import inspect
import itertools
import os
import subprocess

import numpy as np
import pytest

import shape_model as S
from conftest import ROOT
from test_components_cpu import declared
from test_device_edit_cpu import bare_context

FUNCTIONS = ["vxrt_shape_voxels_device"]
HEADER = "vxrt_shape.h"
NEW_SOURCES = ("shape.hip", "api_shape.hip", "shape.h", "shape_rule.h")
CSRC = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")


# ---- the header, the libraries, the wrappers ---------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry_point():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
            assert "vxrt_shape" not in open(os.path.join(ROOT, "include", other)).read(), other      # none of its names elsewhere
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt_transform.h"' in text and "typedef struct vxrt_shape" in text and "typedef enum vxrt_shape_kind" in text
    assert "2^31" in text and "never wrapped" in text and "rint" in text and "half-open" in text
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    assert "api_shape.hip" in open(os.path.join(CSRC, "ctx.h")).read()


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), hdr],
                         capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'typedef char shape_is_32[sizeof(vxrt_shape) == 32 ? 1 : -1];\n'
                   'int main(void) {\n'
                   '    size_t n = 7;\n'
                   '    vxrt_affine a = {{{65536, 0, 0}, {0, 65536, 0}, {0, 0, 65536}}, 0, {0, 0, 0}};\n'
                   '    vxrt_shape s = {VXRT_SHAPE_BALL, 65536, {0, 0, 0}, {0, 0, 0}};\n'
                   '    const int32_t lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};\n'
                   '    const uint8_t mrgb[4] = {1, 2, 3, 4};\n'
                   '    int rc = vxrt_shape_voxels_device(0, &s, &a, lo, hi, mrgb, 0, 0, 0, &n);\n'
                   '    return rc == VXRT_E_INVALID && n == 7 && VXRT_SHAPE_BOX == 0 && VXRT_SHAPE_CYLINDER == 2 && VXRT_SHAPE_CAPSULE == 3 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "vxrt.hpp"\nstatic_assert(sizeof(vxrt_shape) == 32, "vxrt_shape");\n'
                   'size_t f(vxrt::Context& c, const vxrt_shape& s, const vxrt_affine& a, const uint8_t* m, int16_t (*q)[3], uint8_t (*w)[4]) {\n'
                   '    return c.shape_voxels_device(s, a, {0, 0, 0}, {1, 1, 1}) + c.shape_voxels_device(s, a, {0, 0, 0}, {1, 1, 1}, m, q, w, 1)\n'
                   '         + c.shape_voxels_device(s, a, {0, 0, 0}, {1, 1, 1}, nullptr, q, nullptr, 1); }\n')
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
    out_pos = np.full((2, 3), 0x5A5A, np.uint16)
    out_mrgb = np.full((2, 4), 0xA5, np.uint8)
    shape, pull, box_min, box_max = H.ball_shape((0, 0, 0), 1)
    lo, hi = (C.c_int32 * 3)(*box_min), (C.c_int32 * 3)(*box_max)
    mrgb = (C.c_uint8 * 4)(1, 2, 3, 4)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = C.c_size_t(7)
    assert L.vxrt_shape_voxels_device(None, C.byref(shape), C.byref(pull), lo, hi, mrgb, p(out_pos), p(out_mrgb), C.c_size_t(2), C.byref(n)) == H.E_INVALID
    assert L.vxrt_shape_voxels_device(None, C.byref(shape), C.byref(pull), lo, hi, None, None, None, C.c_size_t(0), C.byref(n)) == H.E_INVALID
    assert L.vxrt_shape_voxels_device(None, None, None, None, None, None, None, None, C.c_size_t(0), None) == H.E_INVALID
    assert b"null context" in L.vxrt_last_error()
    assert n.value == 7 and (out_pos == 0x5A5A).all() and (out_mrgb == 0xA5).all()


def test_the_new_sources_are_built_into_both_libraries():
    from gpu_voxel_raytracer_amd import _build
    for f in NEW_SOURCES:
        assert os.path.exists(os.path.join(CSRC, f)), f
    assert "shape.hip" in _build.SOURCES and "api_shape.hip" in _build.SOURCES      # the variants build takes SOURCES too
    assert "shape.h" in _build.HEADERS and "shape_rule.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)
    rule = open(os.path.join(CSRC, "shape_rule.h")).read()
    assert "#include <hip" not in rule and [l for l in rule.splitlines() if l.startswith("#include")] == ['#include "transform_rule.h"']


def test_the_wrapper_signatures(H):
    params = lambda f: list(inspect.signature(f).parameters)      # noqa: E731
    assert params(H.Context.shape_voxels) == ["self", "shape", "pull", "box_min", "box_max", "mrgb", "cap"]
    assert params(H.Context.ball_voxels) == ["self", "center", "radius", "mrgb", "cap"]
    assert params(H.Context.ellipsoid_voxels) == ["self", "center", "radii", "rotation", "mrgb", "cap"]
    assert params(H.Context.box_voxels) == ["self", "center", "half", "rotation", "mrgb", "cap"]
    assert params(H.Context.cylinder_voxels) == params(H.Context.capsule_voxels) == ["self", "a", "b", "radius", "mrgb", "cap"]
    for f in (H.Context.shape_voxels, H.Context.ball_voxels, H.Context.ellipsoid_voxels, H.Context.box_voxels, H.Context.cylinder_voxels, H.Context.capsule_voxels):
        assert inspect.signature(f).parameters["mrgb"].default is None and inspect.signature(f).parameters["cap"].default is None
    assert params(H.ball_shape) == ["center", "radius"] and params(H.ellipsoid_shape) == ["center", "radii", "rotation"]
    assert params(H.box_shape) == ["center", "half", "rotation"] and params(H.cylinder_shape) == params(H.capsule_shape) == ["a", "b", "radius"]
    assert C.sizeof(H.Shape) == 32 and H.Shape.kind.offset == 0 and H.Shape.r.offset == 4 and H.Shape.h.offset == 8 and H.Shape.reserved.offset == 20
    assert (H.SHAPE_BOX, H.SHAPE_BALL, H.SHAPE_CYLINDER, H.SHAPE_CAPSULE) == (0, 1, 2, 3)


def test_the_wrappers_check_their_arguments_before_any_library_call(H):
    ctx = bare_context(H)
    try:
        shape, pull, lo, hi = H.ball_shape((0, 0, 0), 3)
        for bad in (None, 1, "ball", pull, (1, 65536)):
            with pytest.raises(TypeError):
                ctx.shape_voxels(bad, pull, lo, hi)
        for bad in (None, np.eye(3), shape, "pull"):
            with pytest.raises(TypeError):
                ctx.shape_voxels(shape, bad, lo, hi)
        for bad in ((0, 0), (0, 0, 0, 0), (0.5, 0, 0), (32769, 0, 0), (0, -32769, 0), "abc", (None, 0, 0), 3, None):
            with pytest.raises(ValueError):
                ctx.shape_voxels(shape, pull, bad, hi)
            with pytest.raises(ValueError):
                ctx.shape_voxels(shape, pull, lo, bad)
        for bad in ((1, 2, 3), (1, 2, 3, 4, 5), (256, 0, 0, 0), (-1, 0, 0, 0), (0.5, 0, 0, 0), "mrgb", (None, 0, 0, 0), 7):
            with pytest.raises(ValueError):
                ctx.shape_voxels(shape, pull, lo, hi, bad)
            with pytest.raises(ValueError):
                ctx.ball_voxels((0, 0, 0), 3, bad)
        for bad in (-1, 1.5, "3", True):
            with pytest.raises(ValueError):
                ctx.shape_voxels(shape, pull, lo, hi, None, bad)
            with pytest.raises(ValueError):
                ctx.capsule_voxels((0, 0, 0), (5, 5, 5), 2, cap=bad)
        for bad in ((0, 0), (np.inf, 0, 0), "abc", None, (0, 0, 0, 0)):
            for call in (lambda: ctx.ball_voxels(bad, 3), lambda: ctx.ellipsoid_voxels(bad, (1, 2, 3)), lambda: ctx.box_voxels(bad, (1, 2, 3)),
                         lambda: ctx.cylinder_voxels(bad, (1, 2, 3), 2), lambda: ctx.capsule_voxels((1, 2, 3), bad, 2), lambda: ctx.box_voxels((0, 0, 0), bad),
                         lambda: ctx.ellipsoid_voxels((0, 0, 0), bad)):
                with pytest.raises(ValueError):
                    call()
        for bad in (-1, np.nan, np.inf, "3", None, True, 8193):
            for call in (lambda: ctx.ball_voxels((0, 0, 0), bad), lambda: ctx.cylinder_voxels((0, 0, 0), (1, 2, 3), bad), lambda: ctx.capsule_voxels((0, 0, 0), (1, 2, 3), bad)):
                with pytest.raises(ValueError):
                    call()
        for bad in (np.eye(4), np.zeros(9), [[1, 0, 0]] * 2, np.full((3, 3), np.nan)):
            with pytest.raises(ValueError):
                ctx.box_voxels((0, 0, 0), (1, 2, 3), bad)
            with pytest.raises(ValueError):
                ctx.ellipsoid_voxels((0, 0, 0), (1, 2, 3), bad)
        for bad in ((0, 1, 2), (-1, 2, 3), (1, 2, 600), (9000, 9000, 9000)):       # not positive; aspect beyond 256; beyond 8192 cells
            with pytest.raises(ValueError):
                ctx.ellipsoid_voxels((0, 0, 0), bad)
        with pytest.raises(ValueError):
            ctx.box_voxels((0, 0, 0), (1, -2, 3))
        with pytest.raises(ValueError):
            ctx.box_voxels((0, 0, 0), (1, 2, 8193))
        with pytest.raises(ValueError):
            ctx.capsule_voxels((-9000, 0, 0), (9000, 0, 0), 2)                    # h beyond 8192 cells
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


# ---- the model -------------------------------------------------------------------------------------------------------------------
def cells_of(kind, r, h, m, t, lo, hi):
    return {tuple(p) for p in S.shape(kind, r, h, m, t, lo, hi)[0].tolist()}


def ball(radius, centre=(0, 0, 0), grow=2):
    lo, hi = tuple(c - radius - grow for c in centre), tuple(c + radius + grow for c in centre)
    return cells_of(S.BALL, radius * S.ONE, (0, 0, 0), *S.centred(centre), lo, hi)


def test_the_anchors():
    for centre in ((0, 0, 0), (5, -3, 7)):
        one = ball(1, centre)
        assert one == {tuple(c + e for c, e in zip(centre, d)) for d in itertools.product((-1, 0), repeat=3)}      # the 8 cells around that corner
        assert len(ball(2, centre)) == 32 and len(ball(3, centre)) == 136
    pos, _ = S.shape_np(S.BALL, 30 * S.ONE, (0, 0, 0), *S.centred((0, 0, 0)), (-40, -40, -40), (40, 40, 40))
    assert len(pos) == 113104
    cells = {tuple(p) for p in pos.tolist()}
    whole = [o for o in itertools.product(range(-48, 48, 16), repeat=3)
             if all((o[0] + (15 if k & 4 else 0), o[1] + (15 if k & 2 else 0), o[2] + (15 if k & 1 else 0)) in cells for k in range(8))]
    assert len(whole) == 8                                                # the aligned 16^3 tiles wholly inside: those at the centre


def test_the_cube_symmetries_leave_a_centred_ball_invariant():
    for radius in (3, 5):
        for centre in ((0, 0, 0), (2, -1, 4)):
            cells = ball(radius, centre)
            # a cell's centre is c + 1/2: reflecting about the integer centre p sends cell c to 2 p - 1 - c on that axis
            rel = {tuple(2 * (c - p) + 1 for c, p in zip(cell, centre)) for cell in cells}        # odd integers: twice the centre's offset
            count = 0
            for perm in itertools.permutations(range(3)):
                for signs in itertools.product((1, -1), repeat=3):
                    assert {tuple(signs[i] * v[perm[i]] for i in range(3)) for v in rel} == rel
                    count += 1
            assert count == 48


def test_a_box_is_exactly_its_cells_and_abutting_boxes_tile():
    m, t = S.centred((3, -2, 5))
    h = [2 * S.ONE, 4 * S.ONE, 1 * S.ONE]
    got = cells_of(S.BOX, 0, h, m, t, (-10, -10, -10), (12, 12, 12))
    assert got == set(itertools.product(range(1, 5), range(-6, 2), range(4, 6)))
    # two boxes that share the plane x = 7.5 — through cell centres — under a pull that keeps halves: the half-open rule gives each
    # centre on the plane to exactly one of them
    big = (-4, -4, -4), (20, 8, 8)
    left = cells_of(S.BOX, 0, [S.q16(3.5), 2 * S.ONE, 2 * S.ONE], S.identity()[0], [-S.q16(4.0), 0, 0], *big)
    right = cells_of(S.BOX, 0, [S.q16(3.5), 2 * S.ONE, 2 * S.ONE], S.identity()[0], [-S.q16(11.0), 0, 0], *big)
    both = cells_of(S.BOX, 0, [S.q16(7.0), 2 * S.ONE, 2 * S.ONE], S.identity()[0], [-S.q16(7.5), 0, 0], *big)
    assert not left & right and left | right == both and len(both) == 14 * 4 * 4
    assert any(c[0] == 7 for c in right) and not any(c[0] == 7 for c in left)          # the plane's cells: in the box they are the low end of
    # and under a general turn: abutting boxes still partition their union
    from gpu_voxel_raytracer_amd import host as H
    rot = np.array(S_ROTATION)
    a = S.unpack(H, H.box_shape((4, 5, 6), (3, 2, 4), rot))
    lo, hi = a[5], a[6]
    m, t = a[3], a[4]
    shift = 2 * 3 * S.ONE                                                  # the next box along shape x
    first = cells_of(S.BOX, 0, a[2], m, t, lo, (hi[0] + 8, hi[1] + 8, hi[2] + 8))
    second = cells_of(S.BOX, 0, a[2], m, [t[0] - shift, t[1], t[2]], lo, (hi[0] + 8, hi[1] + 8, hi[2] + 8))
    joined = cells_of(S.BOX, 0, [2 * a[2][0], a[2][1], a[2][2]], m, [t[0] - shift // 2, t[1], t[2]], lo, (hi[0] + 8, hi[1] + 8, hi[2] + 8))
    assert not first & second and first | second == joined and len(first) > 150 and len(second) > 150


def _about(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


S_ROTATION = _about((1, 2, 3), np.deg2rad(37.0)).tolist()


def test_inclusions_between_the_kinds_and_growth_with_r():
    from gpu_voxel_raytracer_amd import host as H
    made = S.unpack(H, H.capsule_shape((1, 2, 3), (9, -4, 8), 3.25))
    _, r, h, m, t, lo, hi = made
    capsule = cells_of(S.CAPSULE, r, h, m, t, lo, hi)
    cylinder = cells_of(S.CYLINDER, r, h, m, t, lo, hi)
    assert cylinder < capsule and len(cylinder) > 100
    assert cells_of(S.CAPSULE, r, [0, 0, 0], m, t, lo, hi) == cells_of(S.BALL, r, [0, 0, 0], m, t, lo, hi) < capsule      # h = 0: the ball
    wide = tuple(v - 3 for v in lo), tuple(v + 3 for v in hi)
    for kind, hh in ((S.BALL, [0, 0, 0]), (S.CYLINDER, h), (S.CAPSULE, h)):
        before = set()
        for rr in (0, 1, S.ONE // 2, S.ONE, r, r + 1, r + S.ONE):
            now = cells_of(kind, rr, hh, m, t, *wide)
            assert before <= now, (kind, rr)
            before = now
        assert len(before) > len(cells_of(kind, r, hh, m, t, *wide)) > 0
    # r = 0 and h = 0
    assert not cells_of(S.BOX, 0, [0, S.ONE, S.ONE], *S.centred((0, 0, 0)), (-3, -3, -3), (3, 3, 3))
    assert not cells_of(S.CYLINDER, S.ONE, [0, 0, 0], *S.centred((0, 0, 0)), (-3, -3, -3), (3, 3, 3))
    assert not cells_of(S.BALL, 0, [0, 0, 0], *S.centred((0, 0, 0)), (-3, -3, -3), (3, 3, 3))       # no centre at the corner itself
    assert cells_of(S.BALL, 0, [0, 0, 0], S.identity()[0], [-S.ONE // 2] * 3, (-3, -3, -3), (3, 3, 3)) == {(0, 0, 0)}   # ... but at a centre


def test_the_numpy_walk_equals_the_loop():
    from gpu_voxel_raytracer_amd import host as H
    cases = [H.ball_shape((3.25, -2.5, 7), 6.3), H.ellipsoid_shape((1, 2, 3), (3, 5, 8), S_ROTATION), H.box_shape((0.5, 0, -3), (4, 2.5, 6), S_ROTATION),
             H.cylinder_shape((-3, 2, 1), (6, -4, 9), 2.5), H.capsule_shape((-3, 2, 1), (6, -4, 9), 2.5)]
    for made in cases:
        kind, r, h, m, t, lo, hi = S.unpack(H, made)
        for mrgb in (None, (0x85, 1, 2, 3)):
            want, got = S.shape(kind, r, h, m, t, lo, hi, mrgb), S.shape_np(kind, r, h, m, t, lo, hi, mrgb)
            assert np.array_equal(want[0], got[0]) and len(want[0]) > 100, kind
            assert (want[1] is None and got[1] is None) if mrgb is None else (np.array_equal(want[1], got[1]) and (got[1] == [5, 1, 2, 3]).all())
    # rule 2 in both: the far centre is outside, not wrapped
    far = (S.BALL, S.ONE, [0, 0, 0], [[0] * 3] * 3, [1 << 40, 0, 0], (0, 0, 0), (3, 3, 3))
    assert len(S.shape(*far)[0]) == 0 and len(S.shape_np(*far)[0]) == 0
    assert len(S.shape_np(S.BALL, S.ONE, [0, 0, 0], *S.identity(), (0, 0, 0), (0, 5, 5))[0]) == 0          # an empty box


# ---- the helpers -----------------------------------------------------------------------------------------------------------------
def test_the_helpers_give_the_documented_shapes_maps_and_boxes(H):
    s, a, lo, hi = H.ball_shape((3, -4, 5), 2)
    assert (s.kind, s.r, list(s.h)) == (S.BALL, 2 * S.ONE, [0, 0, 0])
    assert [list(row) for row in a.m] == S.identity()[0] and list(a.t) == [-3 * S.ONE, 4 * S.ONE, -5 * S.ONE]
    assert (lo, hi) == S.helper_box((3, -4, 5), (2, 2, 2)) == ((-1, -8, 1), (7, 0, 9))
    s, a, lo, hi = H.box_shape((0, 0, 0), (1, 2, 3))
    assert (s.kind, s.r, list(s.h)) == (S.BOX, 0, [S.ONE, 2 * S.ONE, 3 * S.ONE]) and (lo, hi) == ((-3, -4, -5), (3, 4, 5))
    s, a, lo, hi = H.capsule_shape((0, 0, -5), (0, 0, 5), 1.5)
    assert (s.kind, s.r, list(s.h)) == (S.CAPSULE, S.q16(1.5), [0, 0, 5 * S.ONE]) and (lo, hi) == S.helper_box((0, 0, 0), (1.5, 1.5, 6.5))
    assert [a.m[2][j] for j in range(3)] == [0, 0, S.ONE]                       # the axis from a to b is shape z
    s, a, lo, hi = H.cylinder_shape((0, -5, 0), (0, 5, 0), 1.5)
    assert (s.kind, s.r, list(s.h)) == (S.CYLINDER, S.q16(1.5), [0, 0, 5 * S.ONE]) and (lo, hi) == S.helper_box((0, 0, 0), (1.5, 5, 1.5))
    assert [a.m[2][j] for j in range(3)] == [0, S.ONE, 0]
    s, a, lo, hi = H.ellipsoid_shape((0, 0, 0), (5, 9, 14))
    assert (s.kind, s.r, list(s.h)) == (S.BALL, 1024 * S.ONE, [0, 0, 0])          # 256 * 5 = 1280 -> 1024
    assert [a.m[i][i] for i in range(3)] == [S.q16(1024 / 5), S.q16(1024 / 9), S.q16(1024 / 14)] and (lo, hi) == S.helper_box((0, 0, 0), (5, 9, 14))
    assert H.ball_shape((32760, 0, -32760), 20)[2:] == ((32738, -22, -32768), (32768, 22, -32738))      # clipped
    assert H.capsule_shape((1, 2, 3), (1, 2, 3), 2)[0].h[2] == 0                  # a == b: the ball


def test_the_helpers_boxes_hold_every_cell_of_the_result(H):
    rng = np.random.default_rng(31)
    cases = []
    for trial in range(4):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        rot = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                        [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                        [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        c = (rng.integers(-30, 30, 3) + rng.random(3)).tolist() if trial < 3 else [20000.25, -15000.5, 32700.75]
        cases.append(("box", H.box_shape(c, (rng.random(3) * 8 + 1).tolist(), rot)))
        cases.append(("ellipsoid", H.ellipsoid_shape(c, (rng.random(3) * 10 + 2).tolist(), rot)))
        b = (np.array(c) + rot[:, 0] * (5 + 10 * rng.random())).tolist()
        cases.append(("capsule", H.capsule_shape(c, b, 1 + 3 * rng.random())))
        cases.append(("cylinder", H.cylinder_shape(c, b, 1 + 3 * rng.random())))
    for name, made in cases:
        kind, r, h, m, t, lo, hi = S.unpack(H, made)
        inner, _ = S.shape_np(kind, r, h, m, t, lo, hi)
        wide = tuple(max(v - 4, -32768) for v in lo), tuple(min(v + 4, 32768) for v in hi)
        outer, _ = S.shape_np(kind, r, h, m, t, *wide)
        assert len(inner) > 20 and np.array_equal(outer, inner), name


# ---- the kernel's arithmetic as a host compiler reads it --------------------------------------------------------------------------
DRIVER = r"""
#include <cstdio>
#include "shape_rule.h"
int main() {
    long long v[20];
    for (;;) {
        for (int k = 0; k < 20; k++)
            if (std::scanf("%lld", &v[k]) != 1) return k == 0 ? 0 : 2;
        int32_t m[3][3], d[3];
        int64_t t[3], p[3], h2[3];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) m[i][j] = int32_t(v[3 * i + j]);
            t[i] = v[9 + i];
            d[i] = int32_t(v[12 + i]);
            h2[i] = 2 * v[17 + i];
        }
        vxrt::shape_pull(m, t, d, p);
        const bool in = vxrt::shape_inside(uint32_t(v[15]), 2 * v[16], h2, p);
        const unsigned long long key = (unsigned long long)vxrt::path_key15(d[0], d[1], d[2]);
        const bool back = int32_t(vxrt::compact16(key >> 2)) - 32768 == d[0] && int32_t(vxrt::compact16(key >> 1)) - 32768 == d[1] &&
                          int32_t(vxrt::compact16(key)) - 32768 == d[2];
        std::printf("%lld %lld %lld %d %d %d\n", (long long)p[0], (long long)p[1], (long long)p[2], vxrt::shape_near(p) ? 1 : 0, in ? 1 : 0, back ? 1 : 0);
    }
}
"""


def build_rule_program(tmp_path):
    """DRIVER around csrc/shape_rule.h under the undefined-behaviour and address sanitizers -> the program's path"""
    src = tmp_path / "rule.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "rule"
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan",
                            "-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


def rule_program_agrees_with_the_model(exe, cases):
    """(m, t, d, kind, r, h) through the program: its output equals the model's and the sanitizers report nothing -> (near, inside) counts"""
    text = "".join(" ".join(str(int(v)) for row in m for v in row) + " " + " ".join(str(int(v)) for v in [*t, *d, kind, r, *h]) + "\n"
                   for m, t, d, kind, r, h in cases)
    run = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), run.stderr[-2000:]
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    near_count = in_count = 0
    for (m, t, d, kind, r, h), line in zip(cases, lines):
        p = S.pulled(m, t, d)
        near = all(abs(v) < S.NEAR for v in p)
        inside = S.holds(kind, r, h, p)
        near_count += near
        in_count += inside
        want = f"{p[0]} {p[1]} {p[2]} {1 if near else 0} {1 if inside else 0} 1"
        assert line == want, (m, t, d, kind, r, h, line, want)
    return near_count, in_count


def test_the_kernels_arithmetic_under_the_sanitizers(tmp_path):
    exe = build_rule_program(tmp_path)
    rng = np.random.default_rng(17)
    big_m, big_t, big = S.M_LIMIT, S.T_LIMIT, S.LIMIT
    kinds = ((S.BOX, 0, [big] * 3), (S.BALL, big, [0] * 3), (S.CYLINDER, big, [0, 0, big]), (S.CAPSULE, big, [0, 0, big]))
    cases = []
    ends = (-32768, -32767, -1, 0, 1, 32766, 32767)
    for kind, r, h in kinds:
        # the limits of the map and of the cell: |P| up to 2^43
        for sm in (big_m, -big_m):
            for st in (big_t, -big_t, 0):
                for d in ends:
                    cases.append(([[sm] * 3] * 3, [st] * 3, [d] * 3, kind, r, h))
                    cases.append(([[sm, -sm, sm], [-sm, -sm, -sm], [0, sm, 0]], [st, -st, st], [d, -1 - d, d], kind, r, h))
        # |P| on both sides of 2^31 on each axis, with the other two at the origin: m = 0, 2 t = P
        for ax in range(3):
            for p in (S.NEAR - 2, S.NEAR, S.NEAR + 2, -S.NEAR + 2, -S.NEAR, -S.NEAR - 2, 1 << 41, -(1 << 41), 1 << 32, (1 << 32) + 2):
                t = [0, 0, 0]
                t[ax] = p // 2
                cases.append(([[0] * 3] * 3, t, [0, 0, 0], kind, r, h))
                cases.append(([[0] * 3] * 3, t, [0, 0, 0], kind, 0 if kind == S.BOX else 1, [1 if v else 0 for v in h]))
        # the shape's own limits: P at +-2^30 (= R = H) and one step past, per axis and on the diagonal
        edge = 1 << 30
        for ax in range(3):
            for p in (edge, edge - 2, edge + 2, -edge, -edge + 2, -edge - 2):
                t = [0, 0, 0]
                t[ax] = p // 2
                cases.append(([[0] * 3] * 3, t, [0, 0, 0], kind, r, h))
        cases.append(([[0] * 3] * 3, [edge // 2 - 1] * 3, [0, 0, 0], kind, r, h))
        cases.append(([[0] * 3] * 3, [S.NEAR // 2 - 1] * 3, [0, 0, 0], kind, r, h))          # three squares just under 2^62 each
    # sums of squares just under and just over R^2: Pythagorean triples scaled to the limit, in P = 2 t
    for a, b, c in ((3, 4, 5), (5, 12, 13), (8, 15, 17), (20, 21, 29)):
        scale = (1 << 30) // c
        rr = c * scale // 2                          # R = 2 r = c * scale
        for da, db in ((0, 0), (2, 0), (0, 2), (-2, 0), (0, -2)):
            t = [(a * scale + da) // 2, (b * scale + db) // 2, 0]
            if c * scale % 2 == 0 and (a * scale) % 2 == 0 and (b * scale) % 2 == 0:
                cases.append(([[0] * 3] * 3, t, [0, 0, 0], S.BALL, rr, [0] * 3))
                cases.append(([[0] * 3] * 3, t, [0, 0, 0], S.CYLINDER, rr, [0, 0, 5]))
                cases.append(([[0] * 3] * 3, [t[0], 0, t[1] + 1000], [0, 0, 0], S.CAPSULE, rr, [0, 0, 1000]))
                cases.append(([[0] * 3] * 3, [t[0], 0, -t[1] - 1000], [0, 0, 0], S.CAPSULE, rr, [0, 0, 1000]))
    # the half-open ends of the box and the cylinder, and the capsule's clamp on both sides
    for p in (-200, -198, 198, 200):
        cases.append(([[0] * 3] * 3, [0, 0, p // 2], [0, 0, 0], S.BOX, 0, [100, 100, 100]))
        cases.append(([[0] * 3] * 3, [p // 2, 0, 0], [0, 0, 0], S.BOX, 0, [100, 100, 100]))
        cases.append(([[0] * 3] * 3, [0, 0, p // 2], [0, 0, 0], S.CYLINDER, 50, [0, 0, 100]))
        cases.append(([[0] * 3] * 3, [0, 0, p // 2 + (50 if p > 0 else -50)], [0, 0, 0], S.CAPSULE, 50, [0, 0, 100]))
        cases.append(([[0] * 3] * 3, [0, 0, p // 2 + (51 if p > 0 else -51)], [0, 0, 0], S.CAPSULE, 50, [0, 0, 100]))
    for _ in range(600):
        kind = int(rng.integers(0, 4))
        wide = rng.random() < 0.3
        m = rng.integers(-big_m if wide else -2 * S.ONE, (big_m if wide else 2 * S.ONE) + 1, (3, 3)).tolist()
        t = rng.integers(-big_t if wide else -(S.ONE << 7), (big_t if wide else S.ONE << 7) + 1, 3).tolist()
        d = rng.integers(-32768 if wide else -200, 32768 if wide else 200, 3).tolist()
        r = 0 if kind == S.BOX else int(rng.integers(0, big + 1 if wide else 300 * S.ONE))
        h = [int(v) for v in rng.integers(0, big + 1 if wide else 300 * S.ONE, 3)]
        h = h if kind == S.BOX else [0, 0, 0] if kind == S.BALL else [0, 0, h[2]]
        cases.append((m, t, d, kind, r, h))
    near_count, in_count = rule_program_agrees_with_the_model(exe, cases)
    assert 100 < near_count < len(cases) - 100 and 100 < in_count < near_count          # every answer of both tests is exercised
