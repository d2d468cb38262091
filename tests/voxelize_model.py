"""The voxeliser's rule (include/vxrt_voxelize.h) in numpy, by brute force over each triangle's candidate cells, and
the meshes the voxeliser's tests share.  Integer arithmetic throughout (int64), so the device's output can be compared bit for bit."""
import numpy as np

Q = 16                      # sixteenths of a voxel
Q_LO, Q_HI = -(1 << 19), 1 << 19


class Refused(Exception):
    """The mesh is refused; .status names the library's status ("invalid" or "scene")."""
    def __init__(self, status, why):
        super().__init__(why)
        self.status = status


def snap(verts):
    """rule 1: q = rint(v * 16) in binary32, round half to even -> int64 (non-finite entries give 0 and are flagged)"""
    v = np.asarray(verts, np.float32).reshape(-1, 3)
    finite = np.isfinite(v)
    with np.errstate(over="ignore", invalid="ignore"):
        r = np.rint(np.where(finite, v, np.float32(0)) * np.float32(Q))
    inside = (r >= np.float32(Q_LO)) & (r < np.float32(Q_HI))
    return np.where(inside, r, 0).astype(np.int64), finite.all(axis=1), inside.all(axis=1)


def cell_range(lo, hi):
    """rule 2, one axis: the least and greatest candidate cell"""
    c0 = lo >> 4
    return c0, (c0 if hi == lo else ((hi + 15) >> 4) - 1)


def triangle_cells(q):
    """rules 2 and 3 for one snapped triangle q int64[3,3] -> the set cells int64[k,3], x fastest ... (any order)"""
    rng = [cell_range(int(q[:, ax].min()), int(q[:, ax].max())) for ax in range(3)]
    out = []
    xs = np.arange(rng[0][0], rng[0][1] + 1, dtype=np.int64)
    ys = np.arange(rng[1][0], rng[1][1] + 1, dtype=np.int64)
    zs = np.arange(rng[2][0], rng[2][1] + 1, dtype=np.int64)
    e = [q[1] - q[0], q[2] - q[1], q[0] - q[2]]
    n = np.cross(e[0], e[1])
    # slabs along z keep the arrays small for the large triangles
    for z0 in range(0, len(zs), 8):
        c = np.stack(np.meshgrid(xs, ys, zs[z0:z0 + 8], indexing="ij"), axis=-1).reshape(-1, 3)
        centre = 16 * c + 8
        v = [q[k][None, :] - centre for k in range(3)]                      # v'_k, [cells, 3]
        ok = np.abs(v[0] @ n) <= 8 * int(np.abs(n).sum())
        for i in range(3):
            axis = np.zeros(3, np.int64)
            axis[i] = 1
            for j in range(3):
                a = np.cross(axis, e[j])
                p = np.stack([v[k] @ a for k in range(3)], axis=0)
                r = 8 * int(np.abs(a).sum())
                ok &= ~((p.min(axis=0) > r) | (p.max(axis=0) < -r))
        out.append(c[ok])
    return np.concatenate(out, axis=0)


def depth_of(pos):
    """the least d with every position inside [-2^d, 2^d)^3"""
    d = 0
    lo, hi = int(pos.min()), int(pos.max())
    while lo < -(1 << d) or hi >= (1 << d):
        d += 1
    return d


def path_keys(pos, depth):
    """the path key of vxrt_get_voxels' order: bit k of u = p + 2^depth lands at bits 3k + 2 (x), 3k + 1 (y), 3k (z)"""
    u = pos.astype(np.int64) + (1 << depth)
    key = np.zeros(len(pos), np.int64)
    for k in range(depth + 1):
        key |= (((u[:, 0] >> k) & 1) << 2 | ((u[:, 1] >> k) & 1) << 1 | ((u[:, 2] >> k) & 1)) << (3 * k)
    return key


def voxelize(verts, tris, mrgb):
    """-> (pos int16[n,3], mrgb uint8[n,4]): unique, in ascending path order, the highest triangle index winning a shared voxel.
    mrgb: one [m, r, g, b] per triangle, or a single one for all."""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    mrgb = np.asarray(mrgb, np.uint8)
    mrgb = np.broadcast_to(mrgb.reshape(-1, 4), (len(tris), 4)) if mrgb.size == 4 else mrgb.reshape(-1, 4)
    assert len(mrgb) == len(tris)
    if len(tris) == 0:
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    if (tris >= len(verts)).any() or (tris < 0).any():
        raise Refused("invalid", "an index is out of range")
    q, finite, inside = snap(verts)
    used = np.unique(tris)
    if not finite[used].all():
        raise Refused("invalid", "a used vertex is not finite")
    if not inside[used].all():
        raise Refused("scene", "a used vertex is outside [-2^19, 2^19) sixteenths")
    cells, owner = [], []
    for t, tri in enumerate(tris):
        c = triangle_cells(q[tri])
        cells.append(c)
        owner.append(np.full(len(c), t, np.int64))
    cells, owner = np.concatenate(cells), np.concatenate(owner)
    if len(cells) == 0:
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    keys = path_keys(cells, depth_of(cells))
    order = np.lexsort((owner, keys))                     # by key, then by triangle index
    keys, cells, owner = keys[order], cells[order], owner[order]
    last = np.r_[keys[1:] != keys[:-1], True]             # the highest triangle index of each key
    out = mrgb[owner[last]].copy()
    out[:, 0] &= 0x7f
    return cells[last].astype(np.int16), out


# ---- meshes -------------------------------------------------------------------------------------------------

def icosphere(subdivisions, radius=10.0, centre=(0.5, 0.5, 0.5)):
    """-> (verts float32[n,3], tris uint32[m,3]): the icosahedron (0, +-1, +-phi) and its cyclic shifts, each triangle split in four
    `subdivisions` times with the new vertices pushed out to the sphere (computed in float64, rounded once)."""
    phi = (1 + 5 ** 0.5) / 2
    v = [(-1, phi, 0), (1, phi, 0), (-1, -phi, 0), (1, -phi, 0), (0, -1, phi), (0, 1, phi), (0, -1, -phi), (0, 1, -phi),
         (phi, 0, -1), (phi, 0, 1), (-phi, 0, -1), (-phi, 0, 1)]
    verts = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    tris = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
            (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nxt = {}, []

        def midpoint(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[k] = len(verts) - 1
            return mid[k]
        for a, b, c in tris:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nxt += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        tris = nxt
    out = np.array(verts) * radius + np.array(centre, np.float64)
    return out.astype(np.float32), np.array(tris, np.uint32)


def cube(lo=0.0, hi=8.0):
    v = np.array([(x, y, z) for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.float32)      # index = 4x + 2y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = [t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))]
    return v, np.array(tris, np.uint32)


def single(*points):
    """a mesh of one triangle over three points"""
    return np.array(points, np.float32), np.array([[0, 1, 2]], np.uint32)


# name -> (mesh, voxel count), the counts of the issue's table
def table():
    seg = ((2.5, 2.5, 2.5), (7.25, 3, -4.5))
    return {
        "icosphere2": (icosphere(2), 1850),
        "cube": (cube(), 361),
        "triangle": (single((1.3, 2.7, 0.2), (9.1, 3.3, 7.9), (4.4, 11.6, 5.5)), 103),
        "segment": (single(seg[0], seg[1], seg[1]), 13),
        "point": (single((3, 3, 3), (3, 3, 3), (3, 3, 3)), 1),
        "large": (single((-150.2, -140.7, 3.1), (149.6, -120.3, -17.4), (-20.9, 151.8, 22.7)), 50619),
        "sliver": (single((-32768, 0.5, 0.5), (32767.9375, 0.5, 0.5), (0, 3.5, 0.5)), 163843),
    }


def concatenated(meshes):
    """several (verts, tris) -> one mesh and a distinct colour per triangle"""
    verts, tris, base = [], [], 0
    for v, t in meshes:
        verts.append(v)
        tris.append(t.astype(np.int64) + base)
        base += len(v)
    tris = np.concatenate(tris).astype(np.uint32)
    k = np.arange(len(tris))
    mrgb = np.stack([k % 128, (k * 7 + 1) % 256, (k * 13 + 2) % 256, (k // 256 + 3) % 256], axis=1).astype(np.uint8)
    return np.concatenate(verts), tris, mrgb
