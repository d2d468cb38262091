"""The solid voxeliser's rule (include/vxrt_solid.h) in numpy and Python integers, by brute force: every triangle
visits every column of its bounds, the crossings are sorted per column in Python, and the union is formed with the surface model
(voxelize_model.py).  Integer arithmetic throughout, so the device's output can be compared bit for bit.  The meshes the solid
voxeliser's tests share are here too."""
import numpy as np

import voxelize_model as M
from voxelize_model import Refused


def snapped(verts, tris):
    """the checks of the surface rule, in its order -> (q int64 [v, 3], tris int64 [t, 3])"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    if (tris >= len(verts)).any() or (tris < 0).any():
        raise Refused("invalid", "an index is out of range")
    q, finite, inside = M.snap(verts)
    used = np.unique(tris)
    if not finite[used].all():
        raise Refused("invalid", "a used vertex is not finite")
    if not inside[used].all():
        raise Refused("scene", "a used vertex is outside [-2^19, 2^19) sixteenths")
    return q, tris


def ceil_div(a, b):
    return -((-a) // b)


def triangle_crossings(q):
    """rules 1 to 3 for one snapped triangle q int64 [3, 3] -> (x, y, k) int64 arrays, one entry per column under the triangle"""
    none = np.zeros(0, np.int64)
    e0, e1 = q[1] - q[0], q[2] - q[1]
    n = np.cross(e0, e1)
    if int(n[2]) == 0:
        return none, none, none
    lo, hi = q.min(axis=0), q.max(axis=0)
    xs = np.arange(ceil_div(int(lo[0]) - 8, 16), (int(hi[0]) - 8) // 16 + 1, dtype=np.int64)      # rule 1
    ys = np.arange(ceil_div(int(lo[1]) - 8, 16), (int(hi[1]) - 8) // 16 + 1, dtype=np.int64)
    if len(xs) == 0 or len(ys) == 0:
        return none, none, none
    x, y = [g.reshape(-1) for g in np.meshgrid(xs, ys, indexing="ij")]
    px, py = 16 * x + 8, 16 * y + 8
    under = np.zeros(len(x), bool)
    for a, b in ((q[0], q[1]), (q[1], q[2]), (q[2], q[0])):                                        # rule 2
        a_in, b_in = a[1] <= py, b[1] <= py
        lx, ly = np.where(a_in, a[0], b[0]), np.where(a_in, a[1], b[1])                            # where it counts, l is the end at or below p
        ux, uy = np.where(a_in, b[0], a[0]), np.where(a_in, b[1], a[1])
        under ^= (a_in != b_in) & ((ux - lx) * (py - ly) - (px - lx) * (uy - ly) > 0)
    x, y, px, py = x[under], y[under], px[under], py[under]
    big = n[0] * (px - q[0][0]) + n[1] * (py - q[0][1]) + n[2] * (8 - q[0][2])                     # rule 3: |A| < 3 * 2^61
    num = -big if n[2] > 0 else big
    return x, y, num // (16 * abs(int(n[2]))) + 1                                                  # numpy's // is the floor


def interior(verts, tris, axis=2):
    """rules 1 to 5 -> the interior cells int64 [n, 3] (sorted by x, y, z), the columns running along `axis` (2, as the rule has
    it; 0 and 1 are for the tests that compare the three).  Raises Refused("scene") with .column and .count for an open mesh."""
    q, tris = snapped(verts, tris)
    roll = {2: [0, 1, 2], 0: [1, 2, 0], 1: [2, 0, 1]}[axis]          # the axes that play x, y, z
    q = q[:, roll]
    columns = {}
    for tri in tris:
        x, y, k = triangle_crossings(q[tri])
        for xi, yi, ki in zip(x.tolist(), y.tolist(), k.tolist()):
            columns.setdefault((xi, yi), []).append(ki)
    cells = []
    for (x, y) in sorted(columns):                                   # x, then y
        ks = sorted(columns[(x, y)])
        if len(ks) % 2:
            e = Refused("scene", f"the mesh is not closed: column ({x}, {y}) is crossed {len(ks)} times")
            e.column, e.count = (x, y), len(ks)
            raise e
        for k0, k1 in zip(ks[0::2], ks[1::2]):
            cells += [(x, y, c) for c in range(k0, k1)]
    out = np.array(cells, np.int64).reshape(-1, 3)
    back = np.argsort(roll)
    return out[:, back]


def solid(verts, tris, mrgb, fill, interior_only=False):
    """-> (pos int16 [n, 3], mrgb uint8 [n, 4]) of vxrt_voxelize_solid_device: unique, in ascending path order.  interior_only: the
    interior cells with the fill bytes (mrgb is not looked at).  Otherwise the surface's voxels with their bytes and the interior
    cells the surface does not set with the fill bytes."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    fill = np.array(fill, np.uint8).reshape(4).copy()
    fill[0] &= 0x7f
    if len(tris) == 0:
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    snapped(verts, tris)                                             # the surface's refusals come first
    inner = interior(verts, tris)
    return compose(None if interior_only else M.voxelize(verts, tris, mrgb), inner, fill)


def compose(surface, inner, fill):
    """The list of solid() from its two parts: the surface's list (pos, mrgb), or None for the interior alone, and the interior's
    cells int64 [n, 3]."""
    fill = np.array(fill, np.uint8).reshape(4).copy()
    fill[0] &= 0x7f
    if surface is None:
        pos, out = inner, np.broadcast_to(fill, (len(inner), 4))
    else:
        spos, smrgb = surface
        have = set(map(tuple, spos.astype(np.int64).tolist()))
        extra = np.array([c for c in map(tuple, inner.tolist()) if c not in have], np.int64).reshape(-1, 3)
        pos = np.concatenate([spos.astype(np.int64), extra])
        out = np.concatenate([smrgb, np.broadcast_to(fill, (len(extra), 4))])
    if len(pos) == 0:
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    # the key's depth does not change the order (DESIGN.md §17 rule 5), so the depth of this list will do
    order = np.argsort(M.path_keys(pos, M.depth_of(pos)), kind="stable")
    return pos[order].astype(np.int16), np.ascontiguousarray(out[order])


# ---- meshes -------------------------------------------------------------------------------------------------

def box(lo, hi):
    """an axis-aligned box, corners lo and hi (3 each, or one number for all axes): 12 triangles"""
    lo, hi = np.broadcast_to(np.asarray(lo, np.float64), 3), np.broadcast_to(np.asarray(hi, np.float64), 3)
    v, t = M.cube(0.0, 1.0)
    return (lo + v.astype(np.float64) * (hi - lo)).astype(np.float32), t


def torus(major=6.0, minor=2.5, nu=12, nv=8, centre=(0.5, 0.5, 0.5)):
    """a torus around the z axis: nu x nv quads, two triangles each"""
    verts = []
    for i in range(nu):
        for j in range(nv):
            a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv
            r = major + minor * np.cos(b)
            verts.append((r * np.cos(a), r * np.sin(a), minor * np.sin(b)))
    tris = []
    for i in range(nu):
        for j in range(nv):
            p, q, r, s = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            tris += [(p, q, r), (p, r, s)]
    return (np.array(verts) + np.array(centre)).astype(np.float32), np.array(tris, np.uint32)


def octahedron(centre=(2.5, 3.5, 0.25), radius=4.0):
    """its top and bottom vertices, and the four around, lie exactly on column centres (centre x, y at c + 0.5, radius whole)"""
    c = np.array(centre, np.float64)
    v = [c + radius * np.array(d, np.float64) for d in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    t = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    return np.array(v, np.float32), np.array(t, np.uint32)


def tetrahedron():
    """every snapped coordinate is 8 (mod 16): every vertex is a cell's centre"""
    v = [(0.5, 0.5, 0.5), (6.5, 1.5, 0.5), (2.5, 7.5, 1.5), (3.5, 2.5, 6.5)]
    return np.array(v, np.float32), np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (2, 0, 3)], np.uint32)


def join(*meshes):
    """several (verts, tris) -> one (verts, tris)"""
    verts, tris, base = [], [], 0
    for v, t in meshes:
        verts.append(np.asarray(v, np.float32))
        tris.append(np.asarray(t, np.int64) + base)
        base += len(v)
    return np.concatenate(verts), np.concatenate(tris).astype(np.uint32)


def slivers(count=300):
    """triangles without a column: each lies between two column centres on x (the centres are at c + 0.5), tilted, none vertical"""
    verts, tris = [], []
    for i in range(count):
        x = float(i % 50)
        verts += [(x + 0.5625, 0.0, i * 0.0625), (x + 0.9375, 0.25, 1.0), (x + 0.625, 5.0, 2.0)]
        tris.append((3 * i, 3 * i + 1, 3 * i + 2))
    return np.array(verts, np.float32), np.array(tris, np.uint32)


def open_cube():
    """the cube [0, 8]^3 without the second triangle of its top face (z = 8)"""
    v, t = M.cube()
    return v, np.delete(t, 11, axis=0)


# name -> (mesh, voxels in UNION mode, voxels in INTERIOR mode): the closed meshes
def table():
    return {
        "icosphere2": (M.icosphere(2), 5065, 3960),
        "torus": (torus(), 1004, 656),
        "cube": (M.cube(), 704, 512),
        "half_box": (box(0.5, 5.5), 216, 125),
        "octahedron": (octahedron(), 209, 88),
        "tetrahedron": (tetrahedron(), 125, 38),
        "nested": (join(M.icosphere(2), M.icosphere(1, radius=5.0)), 4808, 3498),
        "overlapping": (join(M.icosphere(1, radius=6.0), M.icosphere(1, radius=6.0, centre=(5.5, 0.5, 0.5))), 1568, 1004),
    }
