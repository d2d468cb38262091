"""The rule of include/vxrt_mesh.h in Python (no GPU needed), by brute force.

The set is a dict from position to bytes filled in input order, so the last entry of a position wins (transform_model.source_of);
a face is a tuple (d, w, b, c) of Python ints and the faces are sorted as tuples; the runs are one scan over that list; the vertices
are the sorted set of all quads' corners and the triangles index it through a dict.  Also here: six times a mesh's signed volume,
the number of triangles on each edge, and the lists the tests share."""
import numpy as np

from transform_model import HI, LO, source_of

FACES, RUNS = 0, 1
MODES = (FACES, RUNS)
NAMES = ("FACES", "RUNS")
# rule 2: the first six rows of vxrt_morph.h's table
DIRECTIONS = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0))


def axis_of(d):
    return next(a for a in range(3) if DIRECTIONS[d][a])


def faces_of(src):
    """Rule 2 -> [((d, w, b, c), bytes)] ascending by face key, the coordinates as they are (no offset: the order is the same)."""
    out = []
    for p, bytes_ in src.items():
        for d, o in enumerate(DIRECTIONS):
            q = (p[0] + o[0], p[1] + o[1], p[2] + o[2])
            if all(LO <= v <= HI for v in q) and q in src:
                continue
            a = axis_of(d)
            out.append(((d, p[a] + (1 if o[a] > 0 else 0), p[(a + 1) % 3], p[(a + 2) % 3]), bytes_))
    out.sort(key=lambda f: f[0])
    return out


def quads_of(faces, mode, with_bytes):
    """Rule 3 -> [(d, w, b0, c0, c1, bytes)] in the order of their first faces."""
    quads = []
    for i, ((d, w, b, c), bytes_) in enumerate(faces):
        if mode == RUNS and i:
            (pd, pw, pb, pc), pbytes = faces[i - 1]
            if (pd, pw, pb, pc + 1) == (d, w, b, c) and (not with_bytes or pbytes == bytes_):
                quads[-1][4] = c + 1
                continue
        quads.append([d, w, b, c, c + 1, bytes_])
    return [tuple(q) for q in quads]


def corners_of(quad):
    """Rule 4 -> the four corners (x, y, z), counter-clockwise seen from outside."""
    d, w, b0, c0, c1, _ = quad
    b1 = b0 + 1
    a = axis_of(d)
    order = [(b0, c0), (b1, c0), (b1, c1), (b0, c1)] if DIRECTIONS[d][a] > 0 else [(b0, c0), (b0, c1), (b1, c1), (b1, c0)]
    out = []
    for b, c in order:
        p = [0, 0, 0]
        p[a], p[(a + 1) % 3], p[(a + 2) % 3] = w, b, c
        out.append(tuple(p))
    return out


def mesh(pos, mrgb, mode):
    """Rules 1 to 6 -> (verts float32 [V,3], tris uint32 [T,3], tri_mrgb uint8 [T,4] or None)."""
    assert mode in MODES
    src = source_of(np.asarray(pos).reshape(-1, 3), mrgb)
    quads = quads_of(faces_of(src), mode, mrgb is not None)
    corners = [corners_of(q) for q in quads]
    verts = sorted({k for four in corners for k in four})
    index = {k: i for i, k in enumerate(verts)}
    tris, bytes_ = [], []
    for q, (k0, k1, k2, k3) in zip(quads, corners):
        tris += [(index[k0], index[k1], index[k2]), (index[k0], index[k2], index[k3])]
        bytes_ += [q[5], q[5]]
    out_mrgb = None if mrgb is None else np.array(bytes_, np.uint8).reshape(-1, 4)
    return np.array(verts, np.float32).reshape(-1, 3), np.array(tris, np.uint32).reshape(-1, 3), out_mrgb


def quad_areas(pos, mrgb, mode):
    """The quads' areas in unit faces, in their order."""
    src = source_of(np.asarray(pos).reshape(-1, 3), mrgb)
    return [q[4] - q[3] for q in quads_of(faces_of(src), mode, mrgb is not None)]


def volume6(verts, tris):
    """Six times the signed volume of a mesh with integer vertices: the sum of det(v0, v1, v2) over its triangles, in Python ints."""
    v = [[int(c) for c in p] for p in np.asarray(verts).tolist()]
    total = 0
    for i, j, k in np.asarray(tris).tolist():
        a, b, c = v[i], v[j], v[k]
        total += (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]))
    return total


def edge_counts(tris):
    """{(lesser index, greater index): the triangles on that edge}."""
    counts = {}
    for t in np.asarray(tris).tolist():
        for i in range(3):
            e = (min(t[i], t[(i + 1) % 3]), max(t[i], t[(i + 1) % 3]))
            counts[e] = counts.get(e, 0) + 1
    return counts


# ---- the lists the tests share ---------------------------------------------------------------------------------------------------
def cells(*p):
    return np.array(p, np.int16).reshape(-1, 3)


def block(lo, hi):
    """The cells of [lo, hi)^3, or of [lo[a], hi[a]) per axis."""
    lo, hi = np.broadcast_to(np.asarray(lo), 3), np.broadcast_to(np.asarray(hi), 3)
    g = [np.arange(lo[a], hi[a]) for a in range(3)]
    return np.stack(np.meshgrid(*g, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)


def cavity():
    """The 3^3 block without its centre."""
    b = block(-1, 2)
    return b[(b != 0).any(axis=1)]


def bar(axis, length=3000, start=-1500):
    """1 x 1 x length along `axis`, through (5, -7, 3) on the other two."""
    p = np.tile(np.array([5, -7, 3], np.int16), (length, 1))
    p[:, axis] = np.arange(start, start + length)
    return p


def three_colours(n, seed):
    palette = np.array([[1, 200, 10, 10], [2, 10, 200, 10], [0x83, 10, 10, 200]], np.uint8)
    return palette[np.random.default_rng(seed).integers(0, 3, n)]


def one_colour(n):
    return np.tile(np.array([[5, 90, 80, 70]], np.uint8), (n, 1))


def small_families():
    """[(name, pos)]: the lists small enough for the brute-force solid model."""
    rng = np.random.default_rng(27)
    sparse = rng.integers(-4, 5, (40, 3)).astype(np.int16)
    dense = rng.integers(-2, 3, (160, 3)).astype(np.int16)
    return [("one voxel", cells((3, -4, 5))), ("an edge-touching pair", cells((0, 0, 0), (1, 1, 0))), ("a corner-touching pair", cells((0, 0, 0), (1, 1, 1))),
            ("a face-touching pair", cells((0, 0, 0), (0, 0, 1))), ("the block with a cavity", cavity()), ("a slab", block((-3, -2, 0), (4, 3, 2))),
            ("a slab on x", block((2, -3, -3), (3, 3, 4))), ("negative coordinates", block((-9, -8, -7), (-6, -6, -6))),
            ("random sparse", sparse), ("random dense", dense)]
