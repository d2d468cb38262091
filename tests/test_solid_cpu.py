"""CPU: the solid voxeliser's interface (include/vxrt_solid.h) — plain C, declared, exported with C linkage by both libraries, refused
without a context — the Python wrapper's argument checks, which run before any library call, and the numpy model of the interior rule
(solid_model.py) against geometry that does not follow the rule's wording: boxes whose cell counts are known by hand, the same
interior along all three axes, an exact rational ray test of every cell, a flood fill from outside, and the parity rule's answer to
nested and overlapping shells."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import solid_model as S
import voxelize_model as M
from conftest import ROOT

FUNCTIONS = ["vxrt_voxelize_solid_device"]
HEADER = "vxrt_solid.h"
NEW_SOURCES = ("solid.hip", "api_solid.hip", "solid.h")
FILL = (7, 0x10, 0x20, 0x30)
ONE = (3, 0xB0, 0xD0, 0x60)


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vxrt_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_exactly_the_one_entry_point():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt.h"' in text
    assert "parity, not winding" in text
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", hdr], capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '    size_t n = 0;\n'
                   '    const uint8_t fill[4] = {1, 2, 3, 4};\n'
                   '    return vxrt_voxelize_solid_device(0, 0, 0, 0, 0, 0, fill, VXRT_SOLID_INTERIOR, 0, 0, 0, &n) == VXRT_E_INVALID ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)


def test_both_libraries_export_it_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    for lib in (_build.LIB, H.variants_library()):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
        for f in FUNCTIONS:
            assert f in exported, (lib, f)          # unmangled => extern "C"
    assert H.lib().vxrt_abi_version() == 6
    assert (H.SOLID_UNION, H.SOLID_INTERIOR) == (0, 1)


def test_a_null_context_is_invalid(H):
    L = H.lib()
    verts = np.zeros((3, 3), np.float32)
    tris = np.array([[0, 1, 2]], np.uint32)
    mrgb = np.zeros((1, 4), np.uint8)
    fill = (C.c_uint8 * 4)(1, 2, 3, 4)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = C.c_size_t(7)
    for mode in (0, 1, 2):
        assert L.vxrt_voxelize_solid_device(None, p(verts), C.c_size_t(3), p(tris), p(mrgb), C.c_size_t(1), fill, C.c_uint32(mode), None, None,
                                            C.c_size_t(0), C.byref(n)) == H.E_INVALID
        assert L.vxrt_voxelize_solid_device(None, None, C.c_size_t(0), None, None, C.c_size_t(0), None, C.c_uint32(mode), None, None, C.c_size_t(0),
                                            C.byref(n)) == H.E_INVALID
    assert L.vxrt_voxelize_solid_device(None, None, C.c_size_t(0), None, None, C.c_size_t(0), None, C.c_uint32(0), None, None, C.c_size_t(0),
                                        None) == H.E_INVALID
    assert n.value == 7


def test_the_new_sources_do_not_name_the_oracle():
    csrc = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")
    for f in NEW_SOURCES:
        text = open(os.path.join(csrc, f)).read().lower()
        assert "oracle" not in text and "_ref/" not in text, f
    assert "oracle" not in open(os.path.join(ROOT, "include", HEADER)).read().lower()
    from gpu_voxel_raytracer_amd import _build
    assert "solid.hip" in _build.SOURCES and "api_solid.hip" in _build.SOURCES
    assert "solid.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)


class NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def bare_context(H):
    ctx = object.__new__(H.Context)      # no vxrt_create: the checks under test come before any library call
    ctx._L, ctx._h, ctx.device = NoLibrary(), None, 0
    return ctx


def test_the_wrapper_has_the_four_methods(H):
    import inspect
    for name in ("voxelize_solid", "set_solid", "edit_solid", "carve_solid"):
        assert callable(getattr(H.Context, name)), name
    assert list(inspect.signature(H.Context.voxelize_solid).parameters) == ["self", "verts", "tris", "mrgb", "fill", "interior_only", "cap"]
    assert list(inspect.signature(H.Context.carve_solid).parameters) == ["self", "verts", "tris"]
    # the surface's methods keep their signatures
    assert list(inspect.signature(H.Context.voxelize_mesh).parameters) == ["self", "verts", "tris", "mrgb", "cap"]
    assert list(inspect.signature(H.Context.edit_mesh).parameters) == ["self", "verts", "tris", "mrgb", "grow", "cap"]


def test_the_wrapper_checks_its_arguments_before_any_library_call(H):
    import torch
    ctx = bare_context(H)
    try:
        verts, tris, mrgb = np.zeros((5, 3), np.float32), np.zeros((4, 3), np.uint32), np.zeros((4, 4), np.uint8)
        tv = torch.zeros((5, 3), dtype=torch.float32)                    # CPU tensors: the wrong device
        tt, tm = torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 4), dtype=torch.uint8)
        interior = lambda v, t, m, **kw: ctx.voxelize_solid(v, t, m, FILL, interior_only=True, **kw)   # noqa: E731
        with_fill = [lambda v, t, m, f=f, **kw: f(v, t, m, FILL, **kw) for f in (ctx.voxelize_solid, ctx.set_solid, ctx.edit_solid)]
        for call in with_fill + [interior]:
            for bad in (verts.astype(np.float64), verts.astype(np.float16), verts.astype(np.int32), tv.double()):
                with pytest.raises(ValueError):
                    call(bad, tris, mrgb)
            for bad in (tris.astype(np.int16), tris.astype(np.uint64), tris.astype(np.float32), tt.to(torch.int16)):
                with pytest.raises(ValueError):
                    call(verts, bad, mrgb)
            for bad in (mrgb.astype(np.int8), mrgb.astype(np.uint32), tm.to(torch.int32)):
                with pytest.raises(ValueError):
                    call(verts, tris, bad)
            with pytest.raises(ValueError):
                call(verts, tris, mrgb[:3])                               # one mrgb per triangle, or one for all
            with pytest.raises(ValueError):
                call(verts.reshape(-1)[:10], tris, mrgb)                  # not [n, 3]
            with pytest.raises(ValueError):
                call(verts, np.zeros((3, 4), np.uint32), mrgb)
            with pytest.raises(ValueError):
                call(verts, np.array([[0, 1, -2]], np.int64), mrgb[:1])   # an int64 index outside [0, 2^32)
            with pytest.raises(ValueError):
                call(tv, tt, tm)                                          # tensors of another device
            for cap in (-1, 2.5, "9", True):
                with pytest.raises(ValueError):
                    call(verts, tris, mrgb, cap=cap)
            for not_arrays in ((verts.tolist(), tris, mrgb), (verts, None, mrgb), (verts, tris, "mrgb"), (verts, tris, (1, 2, 3, 256))):
                with pytest.raises(TypeError):
                    call(*not_arrays)
        for call in with_fill:
            with pytest.raises(TypeError):
                call(verts, tris, None)                                   # colours may be left out only with interior_only
        for f in (ctx.voxelize_solid, ctx.set_solid, ctx.edit_solid):
            for bad in (None, (1, 2, 3), (1, 2, 3, 256), (1, 2, 3, -1), [1.0, 2, 3, 4], "fill", (True, 2, 3, 4)):
                with pytest.raises(TypeError):
                    f(verts, tris, mrgb, bad)
            for bad in (np.zeros(3, np.uint8), np.zeros(4, np.int32)):
                with pytest.raises(ValueError):
                    f(verts, tris, mrgb, bad)
        with pytest.raises(TypeError):
            ctx.voxelize_solid(verts, tris, mrgb, FILL, interior_only=1)
        for bad in (verts.astype(np.float64), tv):
            with pytest.raises(ValueError):
                ctx.carve_solid(bad, tris)
        with pytest.raises(ValueError):
            ctx.carve_solid(verts, tris.astype(np.int16))
        with pytest.raises(TypeError):
            ctx.carve_solid(verts, None)
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


# ---- the model against geometry ----------------------------------------------------------------------------------------------------
TABLE = S.table()


@pytest.fixture(scope="module")
def inner():
    """name -> the model's interior cells of each mesh of the table, int64 (computed once)"""
    out = {name: S.interior(*mesh) for name, (mesh, _, _) in TABLE.items()}
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def surface():
    """name -> the surface model's cells of each mesh of the table, as a set"""
    return {name: set(map(tuple, M.voxelize(*mesh, ONE)[0].astype(np.int64).tolist())) for name, (mesh, _, _) in TABLE.items()}


def cells_of(a):
    return set(map(tuple, np.asarray(a, np.int64).tolist()))


def block(lo, hi):
    """the cells [lo, hi)^3 (per axis where lo, hi are triples)"""
    lo, hi = np.broadcast_to(lo, 3), np.broadcast_to(hi, 3)
    return {(x, y, z) for x in range(lo[0], hi[0]) for y in range(lo[1], hi[1]) for z in range(lo[2], hi[2])}


@pytest.mark.parametrize("a, b", [(0, 8), (-3, 2), (-7, -6), (5, 6)])
def test_a_box_with_integer_corners_holds_the_cells_between_them(a, b):
    # every centre c + 0.5 with a <= c < b lies strictly inside on all axes, and no other centre is inside or on a face
    assert cells_of(S.interior(*S.box(a, b))) == block(a, b)
    assert cells_of(S.interior(*S.box((a, a, a), (b, b + 1, b + 3)))) == block((a, a, a), (b, b + 1, b + 3))


@pytest.mark.parametrize("a, b", [(0, 5), (-4, -1), (-2, 3)])
def test_a_box_whose_faces_pass_through_cell_centres(a, b):
    # Corners at a + 0.5 and b + 0.5: every face passes through centres, so every face is a tie.
    #   y (rule 2): an edge counts for a_y <= p_y < b_y only, so of the centres a + 0.5 .. b + 0.5 the last is outside: y in [a, b - 1].
    #   x (rule 2): an edge counts when p is strictly on its left (the product is > 0, and 0 on the edge).  A centre on the face
    #      x = a + 0.5 has the far face's edge to its right and its own edge not counted: one crossing, inside.  A centre on the face
    #      x = b + 0.5 has nothing strictly to its right: outside.  x in [a, b - 1].
    #      (The diagonal of a face's two triangles is shared, so it counts twice or not at all.)
    #   z (rule 3): a centre exactly on a plane counts as below it, so the bottom face z = a + 0.5 crosses at k = a + 1 and the top
    #      face z = b + 0.5 at k = b + 1: z in [a + 1, b].
    # (b - a)^3 cells: the box's size, shifted up by one cell on z against x and y.
    got = cells_of(S.interior(*S.box(a + 0.5, b + 0.5)))
    assert got == block((a, a, a + 1), (b, b, b + 1))
    assert len(got) == (b - a) ** 3


@pytest.mark.parametrize("name", ["icosphere2", "torus"])
def test_the_interior_is_the_same_along_every_axis(inner, surface, name):
    mesh = TABLE[name][0]
    along_z = cells_of(inner[name]) - surface[name]
    assert len(along_z) > 100
    for axis in (0, 1):
        assert cells_of(S.interior(*mesh, axis=axis)) - surface[name] == along_z, axis


# Roughly (1, 1, 1), and such that no integer vector w other than 0 with |w_k| < 2^19 is at right angles to it: w . RAY = (w_0 + w_1 +
# w_2) 2^40 + w_1 2^20 + w_2.  A ray from p along RAY meets the line of an edge e through a exactly when RAY . (e x (p - a)) = 0, and
# with coordinates below 2^8.5 sixteenths that cross product is such a w: the ray meets an edge only when p lies on the edge's line.
RAY = ((1 << 40), (1 << 40) + (1 << 20), (1 << 40) + 1)


def ray_says_inside(name, cells):
    """For each cell (int64 [n, 3]) and a mesh of the table: ray_crossings_are_odd, within the bounds the table's meshes keep."""
    verts, tris = TABLE[name][0]
    assert np.abs(M.snap(verts)[0][tris.astype(np.int64)]).max() + 24 < 362 and np.abs(cells).max() < 20
    return ray_crossings_are_odd(verts, tris, cells)


def ray_crossings_are_odd(verts, tris, cells, chunk=256):
    """For each cell (int64 [n, 3]): does the ray from its centre along RAY cross the snapped mesh an odd number of times?  Exact:
    Moller-Trumbore in integers (sixteenths) for every (cell, triangle) pair, vectorised `chunk` cells at a time, which leaves
    u = U / det, v = V / det and t = T / det as integer pairs; the pairs that can be hits at all (|U|, |V| <= |det|) are then decided
    as fractions.Fraction.  A ray through an edge or a vertex would be counted by both neighbours; that is asserted not to happen."""
    q, finite, ok = M.snap(verts)
    tri = q[np.asarray(tris).astype(np.int64)]                       # [t, 3, 3] int64
    d = np.array(RAY, np.int64)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    origin = 16 * np.asarray(cells, np.int64) + 8                    # [n, 3]
    # with E the longest edge component and S the longest cell-to-vertex component, |s x e| <= 2 E S per component: below 2^19 that
    # is RAY's condition, and every sum below stays under 3 * 2^41 * 2^19 < 2^63
    E = int(max(np.abs(e1).max(), np.abs(e2).max()))
    S_ = int(max(np.abs(origin.max(axis=0) - tri.min(axis=(0, 1))).max(), np.abs(origin.min(axis=0) - tri.max(axis=(0, 1))).max()))
    assert 2 * E * max(E, S_) < 1 << 19, (E, S_)
    h = np.cross(d, e2)                                              # [t, 3]
    det = (e1 * h).sum(axis=1)                                       # [t]
    assert (det != 0).all(), "a triangle is parallel to the ray"
    crossings = np.zeros(len(origin), np.int64)
    for c0 in range(0, len(origin), chunk):
        s = origin[c0:c0 + chunk, None, :] - tri[None, :, 0, :]      # [n, t, 3]
        U = (s * h[None]).sum(axis=2)
        qv = np.cross(s, e1[None])
        V = (qv * d).sum(axis=2)
        T = (qv * e2[None]).sum(axis=2)
        maybe = (np.abs(U) <= np.abs(det)[None]) & (np.abs(V) <= np.abs(det)[None])
        for i, t in zip(*np.nonzero(maybe)):
            u, v, w = Fraction(int(U[i, t]), int(det[t])), Fraction(int(V[i, t]), int(det[t])), Fraction(int(T[i, t]), int(det[t]))
            if u < 0 or v < 0 or u + v > 1 or w < 0:
                continue
            assert u > 0 and v > 0 and u + v < 1 and w > 0, "the ray meets an edge, a vertex or starts on the surface"
            crossings[c0 + i] += 1
    return crossings % 2 == 1


@pytest.mark.parametrize("name", ["icosphere2", "torus", "octahedron", "tetrahedron"])
def test_every_interior_cell_is_inside_by_an_exact_ray_test(inner, name):
    # every cell of the interior's bounding box, one cell wider: inside exactly where the rule says so, but for the centres that lie
    # on the surface itself (the octahedron's and the tetrahedron's vertices and edges pass through centres), where the rule's ties
    # decide and a ray test has no answer
    lo, hi = inner[name].min(axis=0) - 1, inner[name].max(axis=0) + 2
    cells = np.array(sorted(block(lo, hi)), np.int64)
    verts, tris = TABLE[name][0]
    q = M.snap(verts)[0][tris.astype(np.int64)]
    n = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    centre = 16 * cells + 8
    on_a_plane = ((centre[:, None, :] - q[None, :, 0, :]) * n[None]).sum(axis=2) == 0        # [cells, t]; a superset of "on the surface"
    free = ~on_a_plane.any(axis=1)
    assert free.sum() > len(cells) // 2
    want = ray_says_inside(name, cells[free])
    have = cells_of(inner[name])
    got = np.array([tuple(c) in have for c in cells[free].tolist()])
    assert np.array_equal(got, want), cells[free][got != want][:5].tolist()
    assert got.sum() > len(have) * 3 // 4


@pytest.mark.parametrize("name", ["icosphere2", "torus", "cube", "half_box", "octahedron", "tetrahedron"])
def test_the_union_has_no_cavity(name):
    pos = S.solid(*TABLE[name][0], ONE, FILL)[0].astype(np.int64)
    lo = pos.min(axis=0) - 1
    size = tuple((pos.max(axis=0) + 2 - lo).tolist())
    wall = np.zeros(size, bool)
    wall[tuple((pos - lo).T)] = True
    seen = np.zeros_like(wall)
    seen[0, 0, 0] = True
    frontier = [(0, 0, 0)]
    while frontier:                                      # 6-connected flood fill from a corner outside the union's bounds
        nxt = []
        for x, y, z in frontier:
            for dx, dy, dz in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                c = (x + dx, y + dy, z + dz)
                if min(c) >= 0 and all(c[k] < size[k] for k in range(3)) and not wall[c] and not seen[c]:
                    seen[c] = True
                    nxt.append(c)
        frontier = nxt
    assert (seen | wall).all(), np.argwhere(~(seen | wall))[:5].tolist()      # every empty cell is reached from outside


def test_nesting_and_overlap_follow_parity(inner, surface):
    # a sphere of radius 5 inside one of radius 10, both about (0.5, 0.5, 0.5): the inner ball is a cavity
    nested = cells_of(inner["nested"])
    outer = cells_of(inner["icosphere2"])
    ball = cells_of(S.interior(*M.icosphere(1, radius=5.0)))
    assert len(ball) > 300 and ball <= outer
    assert nested == outer - ball
    assert (0, 0, 0) not in nested and (0, 0, 7) in nested
    # two spheres of radius 6 about x = 0.5 and x = 5.5: the cells inside both are outside
    a = cells_of(S.interior(*M.icosphere(1, radius=6.0)))
    b = cells_of(S.interior(*M.icosphere(1, radius=6.0, centre=(5.5, 0.5, 0.5))))
    assert len(a & b) > 100
    assert cells_of(inner["overlapping"]) == a ^ b
    assert (3, 0, 0) in a & b and (3, 0, 0) not in cells_of(inner["overlapping"])


@pytest.mark.parametrize("name", ["octahedron", "tetrahedron"])
def test_vertices_on_column_centres_give_even_counts(inner, name):
    verts, tris = TABLE[name][0]
    q = M.snap(verts)[0]
    on_centres = (q[:, :2] % 16 == 8).all(axis=1)
    assert on_centres.all() if name == "octahedron" else (q % 16 == 8).all()
    columns = {}
    for tri in tris.astype(np.int64):
        x, y, k = S.triangle_crossings(q[tri])
        for c in zip(x.tolist(), y.tolist()):
            columns[c] = columns.get(c, 0) + 1
    assert columns and all(v % 2 == 0 for v in columns.values())
    assert len(inner[name]) == TABLE[name][2]


def test_open_meshes_are_refused_with_their_first_odd_column():
    # the cube [0, 8]^3 without the top face's triangle (0, 0) (8, 8) (0, 8), the half of the face above its diagonal x = y: its
    # columns have the bottom face's crossing only.  Rule 2 gives a centre on neither x = 0 nor the diagonal's other side, so the
    # first in x, then y order is (0, 1)
    with pytest.raises(S.Refused) as e:
        S.interior(*S.open_cube())
    assert e.value.status == "scene" and e.value.column == (0, 1) and e.value.count == 1
    tri = M.single((1.3, 2.7, 0.2), (9.1, 3.3, 7.9), (4.4, 11.6, 5.5))
    with pytest.raises(S.Refused) as e:
        S.interior(*tri)
    # the least x with a centre inside is 2 (x = 1.5 lies right of the vertex at 1.3 but outside the narrow tip), and there y = 3
    assert e.value.status == "scene" and e.value.column == (2, 3) and e.value.count == 1
    for interior_only in (False, True):
        with pytest.raises(S.Refused):
            S.solid(*tri, ONE, FILL, interior_only=interior_only)
    # the surface's refusals come first
    v, t = S.open_cube()
    w = v.copy()
    w[0, 0] = np.nan
    with pytest.raises(S.Refused) as e:
        S.solid(w, t, ONE, FILL)
    assert e.value.status == "invalid"
    # triangles without a column cross nothing, open or not
    assert len(S.interior(*S.slivers())) == 0


@pytest.mark.parametrize("name", list(TABLE))
def test_model_counts_and_order(inner, surface, name):
    mesh, union, interior = TABLE[name]
    pos, mrgb = S.solid(*mesh, ONE, FILL)
    ipos, imrgb = S.solid(*mesh, None, (0x87, 1, 2, 3), interior_only=True)
    assert (len(pos), len(ipos)) == (union, interior) and len(inner[name]) == interior
    assert cells_of(ipos) == cells_of(inner[name]) and (imrgb == [7, 1, 2, 3]).all()      # the material's top bit is dropped
    assert cells_of(pos) == cells_of(inner[name]) | surface[name]
    on_surface = np.array([tuple(c) in surface[name] for c in pos.astype(np.int64).tolist()])
    assert (mrgb[on_surface] == ONE).all() and (mrgb[~on_surface] == FILL).all() and (~on_surface).any()
    for p in (pos, ipos):                                # unique, ascending path order at the list's depth and at a deeper one
        for depth in (M.depth_of(p), 15):
            keys = M.path_keys(p, depth)
            assert (keys[1:] > keys[:-1]).all(), depth
