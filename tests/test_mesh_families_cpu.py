"""The mesh families of tests/mesh_families.py are what they claim — checked with the numpy models alone (no GPU, no library).  A
family that stopped tying, stopped reaching the cells past the walk's mask, or stopped having an interior would make the GPU
comparison of tests/test_gpu_mesh_families.py pass for nothing.  The models' lists are cached in mesh_families and shared."""
import numpy as np
import pytest

import mesh_families as F
import solid_model as S
import voxelize_model as M
from test_solid_cpu import ray_crossings_are_odd
from test_voxelize_cpu import samples_on, triangle_distance


def cells_of(a):
    return set(map(tuple, np.asarray(a, np.int64).tolist()))


def assert_same_list(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: positions"
    assert np.array_equal(got[1], want[1]), f"{what}: mrgb"


# ---- the generators ----------------------------------------------------------------------------------------------------------------
def test_families_are_deterministic_and_complete():
    for names, mesh, count in ((F.SURFACE, F.surface_mesh, None), (F.CLOSED, F.closed_mesh, 4 * F.N_TETS)):
        seen = set()
        for name in names:
            v, t, m = mesh(name)
            mesh.cache_clear()
            again = mesh(name)
            for a, b in zip((v, t, m), again):
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
            n = count or (sum(F.N_LONG) if name == "long_segments" else F.N_SURFACE)
            assert v.dtype == np.float32 and t.dtype == np.uint32 and m.dtype == np.uint8
            assert t.shape == (n, 3) and m.shape == (n, 4) and v.shape[1] == 3 and int(t.max()) == len(v) - 1, name
            colours = set(map(tuple, m.tolist()))
            assert len(colours) == n and not colours & seen, name       # a colour per triangle, over the combined mesh too
            seen |= colours
    assert sum(F.N_LONG) == 300
    v, t, m = F.all_surface()
    assert len(t) == (len(F.SURFACE) - 1) * F.N_SURFACE + 300 <= 12300 and len(set(map(tuple, m.tolist()))) == len(t)
    v, t, m = F.all_closed()
    assert len(t) == len(F.CLOSED) * 4 * F.N_TETS and len(set(map(tuple, m.tolist()))) == len(t)


def test_the_triangles_are_small_and_overlap():
    for name in F.SURFACE:
        if name in ("long_segments", "far"):
            continue
        tri = F.snapped_triangles(F.surface_mesh(name))
        assert (tri.max(axis=1) - tri.min(axis=1)).max() <= 16 * 6 + 16, name        # about +-3 voxels round a centre
        assert np.abs(tri).max() <= 16 * 50, name
    # they overlap: the list has fewer voxels than the triangles' own cells add up to, and many colours survive
    for name in ("random", "crowded"):
        pos, mrgb = F.surface_list(name)
        own = sum(len(M.triangle_cells(q)) for q in F.snapped_triangles(F.surface_mesh(name)))
        print(f"surface {name}: {len(pos)} voxels, {own - len(pos)} cells met again, {len(np.unique(mrgb, axis=0))} colours survive")
        assert own - len(pos) >= F.FLOOR["surface", name, "cells met again"], (name, own, len(pos))
        assert len(np.unique(mrgb, axis=0)) > 1000, name


# ---- per-family properties, on the snapped triangles -------------------------------------------------------------------------------
def test_equal_normals_tie_on_the_dominant_axis():
    tri = F.snapped_triangles(F.surface_mesh("equal_normals"))
    share = float(F.dominant_ties(tri).mean())
    print(f"equal_normals: dominant-axis ties {share:.4f}")
    assert share >= F.FLOOR["surface", "equal_normals", "dominant-axis ties"]
    n = np.abs(F.normals(tri))
    n = n[n.any(axis=1)]
    two = (np.sort(n, axis=1)[:, 0] == 0)
    # both kinds, and the tie falls on every pair of axes: x = y, y = z, z = x
    assert two.sum() >= 300 and (~two).sum() >= 400
    for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        assert ((n[:, a] == n[:, b]) & (n[:, c] == 0)).sum() >= 100, (a, b)
    assert float(F.dominant_ties(F.snapped_triangles(F.surface_mesh("random"))).mean()) < 0.02      # a random triangle hardly ever ties


@pytest.mark.parametrize("name", ["degenerate", "long_segments"])
def test_degenerate_families_have_no_normal_at_all(name):
    tri = F.snapped_triangles(F.surface_mesh(name))
    assert not F.normals(tri).any()
    points = (tri == tri[:, :1]).all(axis=(1, 2))
    assert points.sum() >= 30 and (~points).sum() >= 270
    if name == "degenerate":        # all four forms: (a, a, a), (a, b, b), (a, b, a), (a, a, b)
        same = [(tri[:, i] == tri[:, j]).all(axis=1) for i, j in ((0, 1), (1, 2), (2, 0))]
        for form in ((True, True, True), (False, True, False), (False, False, True), (True, False, False)):
            assert np.all([s == f for s, f in zip(same, form)], axis=0).sum() >= 300, form


def test_every_snap_ties_vertex_is_half_way_between_two_sixteenths():
    v = F.surface_mesh("snap_ties")[0]
    product = v * np.float32(16)                    # what the device rounds: exact in binary32
    assert product.dtype == np.float32 and (product.astype(np.float64) == v.astype(np.float64) * 16).all()
    assert (product - np.floor(product) == np.float32(0.5)).all()
    q = M.snap(v)[0]
    assert (q % 2 == 0).all()                       # half to even: every snapped coordinate is even ...
    down = q.astype(np.float64) < product           # ... which rounds some down and some up
    assert 0.4 < down.mean() < 0.6


def test_on_grid_centres_and_corners_lie_where_they_say():
    q = F.snapped_triangles(F.surface_mesh("on_grid")).reshape(-1)
    boundary, centre = float((q % 16 == 0).mean()), float((q % 16 == 8).mean())
    print(f"on_grid: coordinates on a cell boundary {boundary:.4f}, on a centre {centre:.4f}")
    assert boundary >= F.FLOOR["surface", "on_grid", "coordinates on a cell boundary"]
    assert centre >= F.FLOOR["surface", "on_grid", "coordinates on a cell centre"]
    assert (F.snapped_triangles(F.closed_mesh("centres")) % 16 == 8).all()
    assert (F.snapped_triangles(F.closed_mesh("corners")) % 16 == 0).all()
    for name in ("on_grid", "far"):                 # on the snapping grid: the snap changes nothing
        v = F.surface_mesh(name)[0]
        assert (M.snap(v)[0] == v.astype(np.float64) * 16).all()
    for name in ("sixteenths", "flat", "collapsed", "prisms", "far"):
        v = F.closed_mesh(name)[0]
        assert (M.snap(v)[0] == v.astype(np.float64) * 16).all()


def test_axis_planes_are_axis_aligned_and_half_lie_on_a_boundary():
    tri = F.snapped_triangles(F.surface_mesh("axis_planes"))
    shared = (tri == tri[:, :1]).all(axis=1)        # [t, axis]
    assert shared.any(axis=1).all()
    for axis in range(3):
        assert shared[:, axis].sum() >= 400
    on_boundary = float((shared & (tri[:, 0] % 16 == 0)).any(axis=1).mean())
    print(f"axis_planes: planes on a cell boundary {on_boundary:.4f}")
    assert on_boundary >= F.FLOOR["surface", "axis_planes", "planes on a cell boundary"]


def test_long_segments_reach_the_cells_past_the_mask():
    tri = F.snapped_triangles(F.surface_mesh("long_segments"))
    nx, ny, nz, npoints = F.N_LONG
    extent = (tri.max(axis=1) - tri.min(axis=1)) // 16
    assert (extent[:nx, 0] >= 65).all() and (extent[:nx, 0] <= 400).all() and (extent[:nx, 1:] <= 1).all()
    assert (extent[nx:nx + ny, 1] >= 65).all() and (extent[nx + ny:nx + ny + nz, 2] >= 65).all()
    assert (extent[nx:nx + ny + nz, 0] <= 1).all()          # turned along y and z: many columns of a cell or two
    pairs = F.columns_past_the_mask(tri)
    in_list = F.long_columns(F.surface_list("long_segments")[0])
    print(f"long_segments: {pairs} (triangle, column) pairs set a cell 64 or more up the column; {in_list} columns of the list hold more than 64")
    floor = F.FLOOR["surface", "long_segments", "columns past the mask"]
    assert pairs >= floor and in_list >= floor
    # nothing else comes near: no other family has a column of 64 cells
    for name in F.SURFACE:
        if name != "long_segments":
            assert F.columns_past_the_mask(F.snapped_triangles(F.surface_mesh(name))) == 0, name
    # the same voxels from the other end, with the same colours (each segment is one triangle)
    assert_same_list(F.reversed_segments_list(), F.surface_list("long_segments"), "reversed")


def test_far_families_are_at_depth_15_on_both_sides():
    for far, near in ((F.surface_list("far"), F.surface_list("on_grid")), (F.closed_list("far", False), F.closed_list("sixteenths", False)),
                      (F.closed_list("far", True), F.closed_list("sixteenths", True))):
        pos = far[0].astype(np.int64)
        assert M.depth_of(pos) == 15 and pos[:, 0].max() < -16384 and pos[:, 1].min() >= 16384 and pos[:, 2].max() < -16384
        # the same voxels, moved; the path order differs
        assert cells_of(pos) == cells_of(near[0].astype(np.int64) + np.array(F.FAR))
        assert len(pos) == len(near[0])


# ---- closed and open families ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.CLOSED)
def test_closed_families_are_closed_and_have_the_interior_they_claim(name):
    inner = F.closed_interior(name)                 # the model refuses none (it would raise)
    union = F.closed_list(name, False)
    print(f"closed {name}: {len(inner)} interior cells, {len(union[0])} voxels in the union")
    assert len(union[0]) > 0
    if name in F.NO_INTERIOR:
        assert len(inner) == 0 and len(F.closed_list(name, True)[0]) == 0
    else:
        assert len(inner) >= F.INTERIOR_FLOOR[name]
    tri = F.snapped_triangles(F.closed_mesh(name))
    # every edge belongs to an even number of triangles (rule 5's condition)
    edges = {}
    v = F.closed_mesh(name)[0]
    for t in tri:
        for a, b in ((0, 1), (1, 2), (2, 0)):
            key = tuple(sorted((tuple(t[a].tolist()), tuple(t[b].tolist()))))
            if key[0] != key[1]:
                edges[key] = edges.get(key, 0) + 1
    assert all(c % 2 == 0 for c in edges.values())
    nz = F.normals(tri)[:, 2]
    if name == "flat":              # a third of the tetrahedra in each axis plane; the vertical ones cross nothing
        per_tet = (nz.reshape(-1, 4) == 0).all(axis=1)
        assert 250 <= per_tet.sum() <= 280 and not F.normals(tri).reshape(-1, 4, 3).any(axis=1).all(axis=1).any()
    if name == "collapsed":         # two faces without area, and one triangle twice
        assert ((~F.normals(tri).any(axis=1)).reshape(-1, 4).sum(axis=1) >= 2).all()
    if name == "prisms":            # two vertical faces each
        assert ((nz == 0).reshape(-1, 4).sum(axis=1) >= 2).all()


def test_the_shells_overlap_so_parity_decides():
    for name in ("crowded", "sixteenths"):
        v, t, _ = F.closed_mesh(name)
        own = [cells_of(S.interior(v[4 * i:4 * i + 4], F.FACES)) for i in range(F.N_TETS)]
        in_two = sum(len(c) for c in own) - len(set().union(*own))
        print(f"closed {name}: {in_two} cells inside two shells or more")
        if name == "crowded":
            assert in_two >= F.FLOOR["closed", "crowded", "cells inside two shells or more"]
        assert cells_of(F.closed_interior(name)) == cells_of(F.odd_cells([np.array(sorted(c)).reshape(-1, 3) for c in own]))


def test_open_meshes_are_mostly_refused_and_the_model_says_which():
    outcomes = [F.open_outcome(i) for i in range(F.N_OPEN)]
    refused = [o for o in outcomes if o[0] == "refused"]
    accepted = [o for o in outcomes if o[0] == "accepted"]
    print(f"open: {len(refused)} of {F.N_OPEN} refused; crossings {sorted({o[2] for o in refused})}")
    assert len(refused) >= F.FLOOR["open", "refused"] and len(accepted) >= F.FLOOR["open", "accepted"]
    assert len(refused) + len(accepted) == F.N_OPEN
    for kind, column, count in refused:
        assert count % 2 == 1 and len(column) == 2
    assert any(o[2] > 1 for o in refused)           # the count is not always 1
    for i, o in enumerate(outcomes):
        v, t, m = F.open_mesh(i)
        assert len(t) == 4 * F.OPEN_TETS - 1
        if o[0] == "accepted":
            assert len(o[1][0]) > len(o[2][0]) > 0


# ---- independent geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "on_grid", "axis_planes"])
def test_every_sample_on_a_triangle_lies_in_a_set_voxel(name):
    have = cells_of(F.surface_list(name)[0])
    for tri in F.snapped_triangles(F.surface_mesh(name)).astype(np.float64) / 16.0:
        cells = np.unique(np.floor(samples_on(tri)).astype(np.int64), axis=0)
        missed = [c for c in map(tuple, cells.tolist()) if c not in have]
        assert not missed, (name, tri.tolist(), missed[:5])


@pytest.mark.parametrize("name", ["random", "on_grid", "axis_planes"])
def test_every_set_voxel_lies_near_a_triangle(name):
    centres = F.surface_list(name)[0].astype(np.float64) + 0.5
    nearest = np.full(len(centres), np.inf)
    for tri in F.snapped_triangles(F.surface_mesh(name)).astype(np.float64) / 16.0:
        close = np.flatnonzero((np.abs(centres - tri.mean(axis=0)) <= 8.0).all(axis=1))      # the triangle spans at most 6 voxels
        nearest[close] = np.minimum(nearest[close], triangle_distance(centres[close], tri))
    assert nearest.max() <= np.sqrt(3.0) / 2 + 1e-9, (name, float(nearest.max()))


@pytest.mark.parametrize("name", ["random", "crowded"])
def test_the_interior_is_inside_by_an_exact_ray_test_and_the_same_along_every_axis(name):
    v, t, _ = F.closed_mesh(name)
    along = [cells_of(S.interior(v, t, axis=axis)) for axis in (0, 1)] + [cells_of(F.closed_interior(name))]
    have = along[2]
    # every cell that is inside along some axis and its six neighbours, but for the centres that lie on a triangle's plane: there
    # the rule's ties decide, they are along z, and a ray test has no answer
    steps = np.array([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])
    inner = np.array(sorted(along[0] | along[1] | along[2]), np.int64)
    cells = np.unique((inner[:, None, :] + steps[None]).reshape(-1, 3), axis=0)
    q = F.snapped_triangles(F.closed_mesh(name))
    n = F.normals(q)
    assert n.any(axis=1).all()
    on_a_plane = np.zeros(len(cells), bool)
    for k in range(len(q)):
        on_a_plane |= ((16 * cells + 8 - q[k, 0]) @ n[k]) == 0
    free = cells[~on_a_plane]
    assert len(free) > len(cells) * 3 // 4
    want = ray_crossings_are_odd(v, t, free)
    for axis in range(3):
        got = np.array([tuple(c) in along[axis] for c in free.tolist()])
        assert np.array_equal(got, want), (axis, free[got != want][:5].tolist())
    assert want.sum() > len(have) * 3 // 4 and (~want).sum() > len(have) // 2


# ---- the combined meshes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backwards", [False, True], ids=["in order", "backwards"])
def test_all_surface_is_the_merge_of_its_families(backwards):
    direct = M.voxelize(*F.all_surface(backwards))
    assert_same_list(F.all_surface_list(backwards), direct, "all_surface")
    assert len(direct[0]) < sum(len(F.surface_list(k)[0]) for k in F.SURFACE)        # families share voxels
    assert M.depth_of(direct[0]) == 15


def test_the_order_of_the_families_decides_shared_voxels():
    a, b = F.all_surface_list(False), F.all_surface_list(True)
    assert np.array_equal(a[0], b[0])
    assert (a[1] != b[1]).any(axis=1).sum() > 1000


def test_all_closed_is_the_symmetric_difference_of_its_families():
    v, t, m = F.all_closed()
    inner = S.interior(v, t)
    want = F.odd_cells([F.closed_interior(k) for k in F.CLOSED])
    assert np.array_equal(inner, want)              # both sorted by x, y, z
    assert len(want) < sum(len(F.closed_interior(k)) for k in F.CLOSED)              # cells inside two families are outside
    assert_same_list(F.all_closed_list(True), S.compose(None, inner, F.FILL), "all_closed, interior")
    assert_same_list(F.all_closed_list(False), S.compose(M.voxelize(v, t, m), inner, F.FILL), "all_closed, union")
    for mode in (False, True):
        pos = F.all_closed_list(mode)[0]
        keys = M.path_keys(pos, 15)
        assert (keys[1:] > keys[:-1]).all()
