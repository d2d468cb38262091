"""Meshes the two voxelisers dislike, by family, and the models' lists of each (no GPU, no library).

Every family is one mesh (verts float32[v,3], tris uint32[t,3], mrgb uint8[t,4]) of many small triangles with a colour each, spread
over a few dozen voxels so that they overlap and "the highest triangle index wins" is decided thousands of times.  The generators are
seeded and deterministic.  tests/test_mesh_families_cpu.py checks with the models alone that each family is what it claims;
tests/test_gpu_mesh_families.py sends them through the device and compares bit for bit with the lists cached here.

What the families reach that the hand-written tables of voxelize_model.py and solid_model.py do not (csrc/voxelize.hip, solid.hip):
the walk's re-test of cells past its 64-cell mask (`long_segments`), ties on the dominant axis (`equal_normals`), the snap's round
half to even (`snap_ties`), vertices, edges and faces on cell boundaries and centres in bulk (`on_grid`, `axis_planes`, `centres`,
`corners`), closed meshes without volume (`flat`, `collapsed`) or with vertical faces (`prisms`), parity over hundreds of overlapping
shells and the highest triangle index winning a voxel thousands of times (`crowded`), keys at depth 15 (`far`), and the open-mesh
refusal on thirty meshes."""
import functools

import numpy as np

import solid_model as S
import voxelize_model as M

f32 = np.float32
SEED = 20250
N_SURFACE = 1500            # triangles per surface family ...
N_LONG = (150, 60, 60, 30)  # ... but long_segments: segments along x, the first of them turned along y, along z, and points
N_TETS = 400                # tetrahedra per closed family
N_OPEN, OPEN_TETS = 30, 50  # open meshes, and the tetrahedra of each before a triangle is removed
FAR = (-32000, 32000, -32500)
FILL = (0x85, 0x11, 0x22, 0x33)

SURFACE = ("random", "on_grid", "snap_ties", "axis_planes", "equal_normals", "degenerate", "long_segments", "far", "crowded")
CLOSED = ("random", "centres", "corners", "sixteenths", "flat", "collapsed", "prisms", "far", "crowded")

# ---- what the models give with SEED (tests/test_mesh_families_cpu.py asserts it) ---------------------------------------------------
# A property that is a share or a count rather than "all" has a floor: half of what these generators give, rounded down to two digits.
FLOOR = {
    ("surface", "equal_normals", "dominant-axis ties"): 0.49,        # measured 0.997: the rest have no area (random: 0.002)
    ("surface", "on_grid", "coordinates on a cell boundary"): 0.25,  # measured 0.517 of the vertex coordinates
    ("surface", "on_grid", "coordinates on a cell centre"): 0.10,    # measured 0.219
    ("surface", "axis_planes", "planes on a cell boundary"): 0.25,   # measured 0.518 of the triangles
    ("surface", "long_segments", "columns past the mask"): 100,      # the least that the case is for; measured 164 (160 in the list)
    ("surface", "crowded", "cells met again"): 8300,                 # the triangles' own cells less the list's voxels; measured 16764
    ("surface", "random", "cells met again"): 350,                   # measured 711
    ("closed", "crowded", "cells inside two shells or more"): 270,   # measured 542
    ("open", "refused"): N_OPEN // 2,                                # the least that the case is for; measured 26 of 30
    ("open", "accepted"): 1,                                         # measured 4
}
# closed family -> the least interior cells: half the model's count, rounded down to two digits (measured: 2565, 3973, 4353, 3989,
# 2481, 3989, 1809); flat and collapsed have exactly none
INTERIOR_FLOOR = {"random": 1200, "centres": 1900, "corners": 2100, "sixteenths": 1900, "prisms": 1200, "far": 1900, "crowded": 900}
NO_INTERIOR = ("flat", "collapsed")


def colours(first, n):
    """the colour of voxelize_model.concatenated for the triangles first .. first + n - 1 of a combined mesh"""
    k = np.arange(first, first + n)
    return np.stack([k % 128, (k * 7 + 1) % 256, (k * 13 + 2) % 256, (k // 256 + 3) % 256], axis=1).astype(np.uint8)


def _rng(*where):
    return np.random.default_rng([SEED, *where])


def _of_q(q):
    """sixteenths (integers well below 2^24) -> float32, exact"""
    return (np.asarray(q, np.float64) / 16.0).astype(f32)


def _cells(rng, n, k, spread, reach):
    """integer cells int64 [n, k, 3]: within +-reach of a centre drawn from +-spread"""
    return rng.integers(-spread, spread + 1, (n, 1, 3)) + rng.integers(-reach, reach + 1, (n, k, 3))


def _floats(rng, n, k, spread, reach):
    return (rng.uniform(-spread, spread, (n, 1, 3)) + rng.uniform(-reach, reach, (n, k, 3))).astype(f32)


def _sixteenths(rng, n, k, spread, reach):
    return 16 * _cells(rng, n, k, spread, reach) + rng.integers(0, 16, (n, k, 3))


# ---- surface families: points float32 [n, 3, 3] ------------------------------------------------------------------------------------
def _on_grid_q(rng, n):
    cell = _cells(rng, n, 3, 40, 3)
    kind = rng.random((n, 3, 3))
    frac = np.where(kind < 0.5, 0, np.where(kind < 0.7, 8, rng.integers(0, 16, (n, 3, 3))))
    return 16 * cell + frac


def _surface_points(name):
    rng = _rng(0, SURFACE.index(name))
    n = N_SURFACE
    if name == "random":
        return _floats(rng, n, 3, 40, 3)
    if name == "crowded":           # in a box a quarter as wide: most voxels are met by several triangles
        return _floats(rng, n, 3, 10, 3)
    if name == "on_grid":
        return _of_q(_on_grid_q(rng, n))
    if name == "far":               # the triangles of on_grid, moved: whole voxels, so exact
        return _surface_points("on_grid") + np.array(FAR, f32)
    if name == "snap_ties":         # (q + 1/2) / 16 = (2 q + 1) / 32: exact, and so is its product with 16
        q = _sixteenths(rng, n, 3, 40, 3)
        return ((2 * q + 1).astype(np.float64) / 32.0).astype(f32)
    if name == "axis_planes":
        p = _floats(rng, n, 3, 40, 3)
        axis = rng.integers(0, 3, n)
        whole = rng.random(n) < 0.5
        value = np.where(whole, np.rint(p[np.arange(n), 0, axis]), p[np.arange(n), 0, axis]).astype(f32)
        p[np.arange(n), :, axis] = value[:, None]
        return p
    if name == "equal_normals":
        centre = 16 * rng.integers(-40, 41, (n, 3)) + rng.integers(0, 16, (n, 3))
        d = rng.integers(-48, 49, (n, 3, 3))          # the vertices' offsets in sixteenths; one coordinate is overwritten
        kind = np.arange(n) % 7
        for a, b, k in ((0, 1, 0), (1, 2, 1), (2, 0, 2)):          # the plane q_a - q_b = c: |n_a| = |n_b|, the third is zero
            d[kind == k, :, b] = d[kind == k, :, a]
        d[kind >= 3] //= 2                                          # ... as a sum of the other two, which are drawn from half as far
        for k, s in ((3, (1, 1, 1)), (4, (1, 1, -1)), (5, (1, -1, 1)), (6, (-1, 1, 1))):      # s . q = c: |n_x| = |n_y| = |n_z|
            d[kind == k, :, 2] = -s[2] * (s[0] * d[kind == k, :, 0] + s[1] * d[kind == k, :, 1])
        order = np.argsort(rng.random((n, 3)), axis=1)              # every order of the three vertices, so both windings
        d = np.take_along_axis(d, order[:, :, None], axis=1)
        return _of_q(centre[:, None, :] + d)
    if name == "degenerate":
        p = _floats(rng, n, 2, 40, 3)
        a, b = p[:, 0], p[:, 1]
        kind = (np.arange(n) % 4)[:, None, None]
        forms = [np.stack(x, axis=1) for x in ((a, a, a), (a, b, b), (a, b, a), (a, a, b))]
        return np.where(kind == 0, forms[0], np.where(kind == 1, forms[1], np.where(kind == 2, forms[2], forms[3])))
    if name == "long_segments":
        nx, ny, nz, npoints = N_LONG
        a = _sixteenths(rng, nx, 1, 40, 0)[:, 0]
        step = np.stack([16 * rng.integers(65, 400, nx) + rng.integers(0, 16, nx), rng.integers(-4, 5, nx), rng.integers(-4, 5, nx)], axis=1)
        b = a + step                                  # 65 to 400 cells along x, a few sixteenths of slope in y and z
        along_x = np.stack([a, b, b], axis=1)
        along_y = along_x[:ny][:, :, [2, 0, 1]]       # the same segments, x -> y
        along_z = along_x[:nz][:, :, [1, 2, 0]]       # x -> z
        pt = _sixteenths(rng, npoints, 1, 40, 0)
        return _of_q(np.concatenate([along_x, along_y, along_z, np.repeat(pt, 3, axis=1)]))
    raise KeyError(name)


def _first_triangle(names, name, per_family):
    return sum(per_family(k) for k in names[:names.index(name)])


def _surface_count(name):
    return sum(N_LONG) if name == "long_segments" else N_SURFACE


@functools.lru_cache(maxsize=None)
def surface_mesh(name):
    """-> (verts, tris, mrgb) of a surface family.  The colours are those of the family's place in all_surface, so that the
    family's list is a part of the combined one."""
    p = _surface_points(name)
    n = len(p)
    assert p.dtype == f32 and n == _surface_count(name)
    out = (p.reshape(-1, 3).copy(), np.arange(3 * n, dtype=np.uint32).reshape(n, 3), colours(_first_triangle(SURFACE, name, _surface_count), n))
    for a in out:
        a.setflags(write=False)
    return out


def reversed_segments(mesh):
    """(a, b, b) -> (b, a, a) for every triangle: the same segments and points from the other end"""
    v, t, m = mesh
    return v, np.ascontiguousarray(t[:, [1, 0, 0]]), m


# ---- closed families: tetrahedra, points float32 [n, 4, 3] ------------------------------------------------------------------------
FACES = np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)], np.int64)      # as solid_model.tetrahedron


def _tetrahedra_q(rng, n):
    return _sixteenths(rng, n, 4, 30, 4)


def _closed_points(name):
    rng = _rng(1, CLOSED.index(name))
    n = N_TETS
    if name == "random":
        return _floats(rng, n, 4, 30, 4)
    if name == "crowded":           # in a box a quarter as wide: most interior cells lie inside several shells
        return _floats(rng, n, 4, 8, 4)
    if name == "centres":
        return _of_q(16 * _cells(rng, n, 4, 30, 4) + 8)
    if name == "corners":
        return _of_q(16 * _cells(rng, n, 4, 30, 4))
    if name == "sixteenths":
        return _of_q(_tetrahedra_q(rng, n))
    if name == "far":
        return _closed_points("sixteenths") + np.array(FAR, f32)
    q = _tetrahedra_q(rng, n)
    i = np.arange(n)
    if name == "flat":              # four points of one axis plane: x = c and y = c (vertical) and z = c in turn
        axis = i % 3
        q[i, :, axis] = q[i, 0, axis][:, None]
    elif name == "collapsed":       # two of the four vertices are the same point
        pair = np.argsort(rng.random((n, 4)), axis=1)[:, :2]
        q[i, pair[:, 1]] = q[i, pair[:, 0]]
    elif name == "prisms":          # two vertices share x and y: the two faces on that edge have n_z = 0
        pair = np.argsort(rng.random((n, 4)), axis=1)[:, :2]
        q[i, pair[:, 1], :2] = q[i, pair[:, 0], :2]
    else:
        raise KeyError(name)
    return _of_q(q)


def _tetrahedra_mesh(p, first_triangle):
    n = len(p)
    tris = (4 * np.arange(n)[:, None, None] + FACES[None]).reshape(-1, 3).astype(np.uint32)
    return p.reshape(-1, 3).copy(), tris, colours(first_triangle, len(tris))


@functools.lru_cache(maxsize=None)
def closed_mesh(name):
    """-> (verts, tris, mrgb) of a closed family, coloured by its place in all_closed"""
    out = _tetrahedra_mesh(_closed_points(name), _first_triangle(CLOSED, name, lambda k: 4 * N_TETS))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def open_mesh(i):
    """-> (verts, tris, mrgb): OPEN_TETS tetrahedra on sixteenths without one of their triangles"""
    rng = _rng(2, i)
    v, t, m = _tetrahedra_mesh(_of_q(_tetrahedra_q(rng, OPEN_TETS)), 0)
    gone = int(rng.integers(0, len(t)))
    return v, np.delete(t, gone, axis=0), np.delete(m, gone, axis=0)


# ---- combined meshes ---------------------------------------------------------------------------------------------------------------
def concatenated(meshes):
    """several (verts, tris, mrgb) -> one, each triangle keeping its colour"""
    verts, tris, mrgb, base = [], [], [], 0
    for v, t, m in meshes:
        verts.append(v)
        tris.append(t.astype(np.int64) + base)
        mrgb.append(m)
        base += len(v)
    return np.concatenate(verts), np.concatenate(tris).astype(np.uint32), np.concatenate(mrgb)


@functools.lru_cache(maxsize=None)
def all_surface(backwards=False):
    """every surface family in one mesh, in the order of SURFACE or the other way round"""
    return concatenated([surface_mesh(k) for k in (SURFACE[::-1] if backwards else SURFACE)])


@functools.lru_cache(maxsize=None)
def all_closed():
    return concatenated([closed_mesh(k) for k in CLOSED])


# ---- the models' lists, computed once ----------------------------------------------------------------------------------------------
def _frozen(pos, mrgb):
    pos.setflags(write=False)
    mrgb.setflags(write=False)
    return pos, mrgb


@functools.lru_cache(maxsize=None)
def surface_list(name):
    return _frozen(*M.voxelize(*surface_mesh(name)))


@functools.lru_cache(maxsize=None)
def reversed_segments_list():
    return _frozen(*M.voxelize(*reversed_segments(surface_mesh("long_segments"))))


@functools.lru_cache(maxsize=None)
def closed_surface_list(name):
    return _frozen(*M.voxelize(*closed_mesh(name)))


@functools.lru_cache(maxsize=None)
def closed_interior(name):
    """the interior cells int64 [n, 3]; no closed family is refused"""
    v, t, _ = closed_mesh(name)
    inner = S.interior(v, t)
    inner.setflags(write=False)
    return inner


@functools.lru_cache(maxsize=None)
def closed_list(name, interior_only):
    return _frozen(*S.compose(None if interior_only else closed_surface_list(name), closed_interior(name), FILL))


def merged(lists):
    """Surface lists of meshes concatenated in this order -> the list of the whole: a later mesh's triangles have the higher
    indices, so it wins a shared voxel; then path order at the merged depth."""
    pos = np.concatenate([p for p, _ in lists]).astype(np.int64)
    mrgb = np.concatenate([m for _, m in lists])
    if len(pos) == 0:
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    rank = np.concatenate([np.full(len(p), i) for i, (p, _) in enumerate(lists)])
    keys = M.path_keys(pos, M.depth_of(pos))
    order = np.lexsort((rank, keys))
    keys, pos, mrgb = keys[order], pos[order], mrgb[order]
    last = np.r_[keys[1:] != keys[:-1], True]
    return pos[last].astype(np.int16), np.ascontiguousarray(mrgb[last])


def odd_cells(interiors):
    """Interiors of shells voxelised together: a column's crossings are sorted together and a cell is inside iff an odd number lie at
    or below it, so the whole's interior is the symmetric difference of the parts' -> int64 [n, 3], sorted by x, y, z"""
    cells = np.concatenate([np.asarray(c, np.int64).reshape(-1, 3) for c in interiors])
    if len(cells) == 0:
        return cells
    uniq, count = np.unique(cells, axis=0, return_counts=True)
    return uniq[count % 2 == 1]


@functools.lru_cache(maxsize=None)
def all_surface_list(backwards=False):
    return _frozen(*merged([surface_list(k) for k in (SURFACE[::-1] if backwards else SURFACE)]))


@functools.lru_cache(maxsize=None)
def all_closed_list(interior_only):
    inner = odd_cells([closed_interior(k) for k in CLOSED])
    surface = None if interior_only else merged([closed_surface_list(k) for k in CLOSED])
    return _frozen(*S.compose(surface, inner, FILL))


@functools.lru_cache(maxsize=None)
def open_outcome(i):
    """What the model says of open mesh i: ("refused", (x, y), crossings), or ("accepted", union list, interior list) where the
    removed triangle crossed no column."""
    v, t, m = open_mesh(i)
    try:
        inner = S.interior(v, t)
    except S.Refused as e:
        assert e.status == "scene"
        return "refused", e.column, e.count
    return "accepted", _frozen(*S.compose(M.voxelize(v, t, m), inner, FILL)), _frozen(*S.compose(None, inner, FILL))


# ---- what a family claims, measured on the snapped triangles -----------------------------------------------------------------------
def snapped_triangles(mesh):
    """-> int64 [t, 3, 3], sixteenths"""
    v, t, _ = mesh
    q, finite, inside = M.snap(v)
    assert finite.all() and inside.all()
    return q[t.astype(np.int64)]


def normals(tri):
    return np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1])


def dominant_ties(tri):
    """bool [t]: the greatest |n_a| is not zero and two axes or three have it"""
    n = np.abs(normals(tri))
    top = n.max(axis=1)
    return (top > 0) & ((n == top[:, None]).sum(axis=1) >= 2)


def columns_past_the_mask(tri):
    """The (triangle, column) pairs of zero-normal triangles that set a cell 64 or more cells up their column: the cells the walk's
    emit pass tests a second time.  Such a triangle's columns run along x from its least candidate cell (csrc/voxelize.hip: d = 0)."""
    pairs = 0
    for q in tri:
        if np.any(np.cross(q[1] - q[0], q[2] - q[1])) or int(q[:, 0].max() - q[:, 0].min()) < 64 * 16:
            continue
        cells = M.triangle_cells(q)
        past = cells[cells[:, 0] - M.cell_range(int(q[:, 0].min()), int(q[:, 0].max()))[0] >= 64]
        pairs += len(np.unique(past[:, 1:], axis=0))
    return pairs


def long_columns(pos):
    """the columns along x of a voxel list (a y and a z) that hold more than 64 voxels"""
    _, count = np.unique(np.asarray(pos)[:, 1:], axis=0, return_counts=True)
    return int((count > 64).sum())
