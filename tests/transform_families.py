"""Maps, lists and boxes the list resampler dislikes, by family, and the model's result of each (no GPU, no library).

A family is a tuple of cases `Case(name, pos, mrgb, m, t, box_min, box_max)`, made per list kind: "from_map", a list made from the
case's own map and box, and "fixed", one of the lists below with `t` solved in integers so that a chosen cell of the box pulls a
chosen voxel of the list (`solve_t`; a draw whose `t` would pass 2^40 is redrawn).  The generators are seeded and deterministic;
the expected result of a case is `transform_model.transform_np`'s walk of its whole box, cached (`expected`).
tests/test_transform_families_cpu.py checks with the models alone that each family is what it claims;
tests/test_gpu_transform_families.py sends them through the device.

The module also restates, in Python integers, how csrc/transform.hip deals a box's cells to blocks (`blocks`) and the block cull's
interval rule (`cull`).  That restatement only CLASSIFIES cases — which blocks the cull drops, and by how many cells a block's
interval clears the source's bounding box — and places the `near_miss` maps; it never predicts a byte of output.

What could not be built as the families were first described, and why:
* an overshoot of 2^32 cells.  With |m| <= 2^24, |t| <= 2^40 and |2 d + 1| < 2^17 every |P| is below 2^43, so |s| < 2^26: s never
  leaves 32 bits.  `past_range` overshoots by 1 to 3 cells, by exactly 2^16 cells and by exactly 2^24 cells (t = +-2^40, the
  farthest multiple of 2^16 a map can reach); the last two also wrap a P held in 32 bits (2^16 cells are 2^33 in P) onto the
  same voxel.  The CPU file counts the wraps of s in 16 bits and of P in 32 bits.
* `clustered` has about 4 300 unique cells, not 5 000: a 16^3 cube has 4 096 cells, and nine tenths of the list lie in it.
* `from_map` lists the pulled cells of a random third of the DISTINCT source cells the box pulls, not of a third of the box's
  cells: under a magnifying or singular map a third of the cells pull every one of them, and the result would be the whole box.
* `rigid` has no box with a z run over 2 048 cells: rigid_box of a list is that long only for a rod, and under a uniformly drawn
  rotation a rod's box is far over the 300 000 cells allowed here.  Its blocks are rows and slabs."""
import functools
import itertools
from typing import NamedTuple

import numpy as np

import transform_model as T

SEED = 2311
SPAN = 2048                         # csrc/transform.h: kPullSpan, the cells of a block
STAGED = 1024                       # kPullSample, the staged keys
ONE = T.ONE
FAMILIES = ("limits", "magnify", "minify", "shear", "singular", "mirror", "ties", "past_range", "rigid", "near_miss")
KINDS = ("from_map", "fixed")
MAX_BOX, MAX_TOTAL = 300_000, 12_000_000

# ---- what the generators give with SEED (tests/test_transform_families_cpu.py asserts it) ------------------------------------------
# A claim that is a count or a share has a floor: half of what these generators give, rounded down to two digits
# (mesh_families.FLOOR's convention).
FLOOR = {
    ("from_map", "share of listed voxels that no cell pulls"): 0.21,                  # measured 0.423 (limits, minify and shear)
    ("ties", "share of cells with P = 0 mod 2^17 on some axis"): 0.39,                # measured 0.787
    ("ties", "share of cells with a negative P"): 0.46,                               # measured 0.938
    ("ties", "share of cells where a truncation is not the floor"): 0.29,             # measured 0.588
    ("past_range", "cells whose s wraps onto a listed voxel in 16 bits"): 1300,       # measured 2738
    ("past_range", "cells whose P wraps onto a listed voxel in 32 bits"): 590,        # measured 1184
    ("singular", "most cells that pull one voxel"): 10000,                            # measured 20 520 (m = 0: the whole box)
    ("singular", "most cells that pull one voxel, rank 1 and 2"): 160,                # measured 325 (rank 1) and 2 220 (rank 2)
    ("clustered", "staged sample indices inside the cluster"): 450,                   # measured 918 of 1 024
    ("clustered", "box cells whose key lies strictly between two clusters"): 26000,   # measured 53 519 in 9 boxes
    ("limits", "greatest |P| in bits"): 42,                                           # the least that the family is for; measured 42
    ("magnify", "blocks whose every cell hits"): 6,                                   # measured 12
    # a ceiling, not a floor, and reasoned: a from_map list holds a third of what the box pulls and at most as many decoys
    ("minify", "greatest share of a box that hits"): 0.67,                            # measured 0.362
}


class Case(NamedTuple):
    name: str
    pos: np.ndarray
    mrgb: np.ndarray
    m: list
    t: list
    box_min: tuple
    box_max: tuple


def _rng(*where):
    return np.random.default_rng([SEED, *where])


# ---- the block layout and the cull, restated (classification only) ------------------------------------------------------------------
def extents(box_min, box_max):
    return tuple(max(0, int(b) - int(a)) for a, b in zip(box_min, box_max))


def cell_of(box_min, ext, c):
    """transform.hip: cell_of — cell c of the box is box_min + (c / (ey ez), c / ez % ey, c % ez)."""
    yz = ext[1] * ext[2]
    return (int(box_min[0]) + c // yz, int(box_min[1]) + c % yz // ext[2], int(box_min[2]) + c % ext[2])


def blocks(box_min, box_max):
    """-> [(shape, lo, hi)] per block of SPAN consecutive cells: the box of cells the cull takes for it (inclusive corners) and its
    shape: "run" (inside one z run), "rows" (whole z rows of one x) or "slab" (whole x slabs)."""
    ext = extents(box_min, box_max)
    cells = ext[0] * ext[1] * ext[2]
    out = []
    for c0 in range(0, cells, SPAN):
        p, q = cell_of(box_min, ext, c0), cell_of(box_min, ext, min(c0 + SPAN, cells) - 1)
        lo = [p[0], int(box_min[1]), int(box_min[2])]
        hi = [q[0], int(box_min[1]) + ext[1] - 1, int(box_min[2]) + ext[2] - 1]
        shape = "slab"
        if p[0] == q[0]:
            lo[1], hi[1], shape = p[1], q[1], "rows"
            if p[1] == q[1]:
                lo[2], hi[2], shape = p[2], q[2], "run"
        out.append((shape, tuple(lo), tuple(hi)))
    return out


def interval(m, t, lo, hi, i):
    """The cull's interval of s on source axis i over the cells lo .. hi: the floors of the sums of the terms' least and greatest."""
    least = most = 2 * int(t[i])
    for j in range(3):
        u, v = int(m[i][j]) * (2 * lo[j] + 1), int(m[i][j]) * (2 * hi[j] + 1)
        least, most = least + min(u, v), most + max(u, v)
    return least >> 17, most >> 17


def bounds(pos):
    p = np.asarray(pos, np.int64).reshape(-1, 3)
    return tuple(int(v) for v in p.min(0)), tuple(int(v) for v in p.max(0))


def cull(case):
    """-> [(shape, dropped, below, above)] per block: below[i] = src_lo[i] - the interval's greatest s, above[i] = the interval's
    least s - src_hi[i], in cells.  A block is dropped when any of the six is positive: 1 is one cell short of the source's
    bounding box, 0 exactly on its edge, -1 one cell inside."""
    src_lo, src_hi = bounds(case.pos)
    out = []
    for shape, lo, hi in blocks(case.box_min, case.box_max):
        iv = [interval(case.m, case.t, lo, hi, i) for i in range(3)]
        below = tuple(src_lo[i] - iv[i][1] for i in range(3))
        above = tuple(iv[i][0] - src_hi[i] for i in range(3))
        out.append((shape, any(v > 0 for v in below + above), below, above))
    return out


# ---- the pull of a whole box in numpy int64 (exact: |P| < 2^43) ----------------------------------------------------------------------
def box_cells(box_min, box_max):
    axes = [np.arange(int(box_min[ax]), int(box_max[ax]), dtype=np.int64) for ax in range(3)]
    return np.stack(np.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)


def pulled(m, t, cells):
    """-> (P int64 [k,3], s int64 [k,3], in range bool [k]) of rule 2 and rule 3's range test."""
    p = (2 * cells + 1) @ np.array(m, np.int64).T + 2 * np.array(t, np.int64)
    s = p >> 17
    return p, s, ((s >= T.LO) & (s <= T.HI)).all(axis=1)


def keys_of(a):
    return (a[:, 0] + 32768) << 32 | (a[:, 1] + 32768) << 16 | (a[:, 2] + 32768)


def path_keys(a):
    """transform_model.path_key at depth 15 of int64 [k,3] positions of the int16 range, in numpy (for classifying cases)"""
    def spread(v):
        x = v & 0xFFFF
        x = (x | x << 16) & 0x0000FF0000FF
        x = (x | x << 8) & 0x00F00F00F00F
        x = (x | x << 4) & 0x0C30C30C30C3
        return (x | x << 2) & 0x249249249249
    u = np.asarray(a, np.int64).reshape(-1, 3) + 32768
    return spread(u[:, 0]) << 2 | spread(u[:, 1]) << 1 | spread(u[:, 2])


def hits(pos, m, t, box_min, box_max):
    """how many cells of the box pull a listed voxel (for classifying a draw; the expected output is the model's)"""
    _, s, ok = pulled(m, t, box_cells(box_min, box_max))
    return int(np.isin(keys_of(s[ok]), keys_of(np.asarray(pos, np.int64).reshape(-1, 3))).sum())


def solve_t(m, cell, voxel, rest=None):
    """t in integers such that `cell` pulls `voxel`: P_i = voxel_i 2^17 + r with r the middle of the cell, or `rest` where the
    family wants P on a boundary (rest must have P's parity) -> [t0, t1, t2], or None when a |t| would pass 2^40."""
    t = []
    for i in range(3):
        x = sum(int(m[i][j]) * (2 * int(cell[j]) + 1) for j in range(3))
        r = (ONE + ((x + ONE) & 1)) if rest is None else rest(x)
        assert (r - x) % 2 == 0 and 0 <= r < 2 * ONE
        t.append(((int(voxel[i]) << 17) + r - x) // 2)
    return None if any(abs(v) > T.T_LIMIT for v in t) else t


# ---- source lists: random bytes, 5 % of the positions listed twice with other bytes, shuffled ------------------------------------------
def _listed(rng, cells):
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    cells = np.unique(cells, axis=0)
    assert len(cells) and cells.min() >= T.LO and cells.max() <= T.HI
    cells = np.concatenate([cells, cells[rng.integers(0, len(cells), max(1, len(cells) // 20))]])
    cells = cells[rng.permutation(len(cells))]
    return cells.astype(np.int16), rng.integers(0, 256, (len(cells), 4)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def blob():
    """transform_model.random_cells() moved to straddle 0 on all axes: [-20, 20)^3"""
    pos, mrgb = T.random_cells()
    return (pos.astype(np.int64) - 20).astype(np.int16), mrgb


@functools.lru_cache(maxsize=None)
def small_blob():
    """blob's entries in [-12, 12)^3, for the rigid motions (their box grows with the list's diagonal)"""
    pos, mrgb = blob()
    keep = (np.abs(pos.astype(np.int64) * 2 + 1) < 24).all(axis=1)
    return pos[keep], mrgb[keep]


CORNERS = tuple(itertools.product((T.LO, T.HI), repeat=3))


@functools.lru_cache(maxsize=None)
def far():
    """About 200 cells of the 6^3 cube at each of the eight int16 corners and around the origin: the bounds are the whole range and
    the keys use all 48 bits.  past_range relies on the cubes: a coordinate wrapped past one end lands in the cube at the other."""
    rng = _rng(1, 1)
    g = np.arange(6)
    cube = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    parts = []
    for c in CORNERS + ((-3, -3, -3),):
        at = np.array([v if v <= 0 else v - 5 for v in c]) + cube
        parts.append(at[rng.random(len(at)) < 0.93])
    return _listed(rng, np.concatenate(parts))


CLUSTER_AT = (100, -200, 300)


@functools.lru_cache(maxsize=None)
def clustered():
    """Nine tenths in the cube CLUSTER_AT + [0, 16)^3, the rest singles over [-30000, 30000]^3."""
    rng = _rng(1, 2)
    g = np.arange(16)
    cube = np.array(CLUSTER_AT) + np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    cube = cube[rng.random(len(cube)) < 0.9]
    return _listed(rng, np.concatenate([cube, rng.integers(-30000, 30001, (430, 3))]))


@functools.lru_cache(maxsize=None)
def line():
    """One run along z at (3, -4): the bounding box is degenerate on two axes."""
    rng = _rng(1, 3)
    z = np.arange(-1200, 1200)[rng.random(2400) < 0.7]
    return _listed(rng, np.stack([np.full(len(z), 3), np.full(len(z), -4), z], -1))


@functools.lru_cache(maxsize=None)
def plane():
    """One sheet at x = 7 over y in [-40, 40), z in [-1100, 1100): the bounding box is degenerate on one axis."""
    rng = _rng(1, 4)
    y, z = np.meshgrid(np.arange(-40, 40), np.arange(-1100, 1100), indexing="ij")
    keep = rng.random(y.shape) < 0.15
    return _listed(rng, np.stack([np.full(int(keep.sum()), 7), y[keep], z[keep]], -1))


NEAR = {"far": (0, 0, 0), "clustered": tuple(v + 8 for v in CLUSTER_AT)}          # where middle_voxel looks in these two
FIXED = {"blob": blob, "small_blob": small_blob, "far": far, "clustered": clustered, "line": line, "plane": plane}


def middle_voxel(pos, rng, near=None):
    """a listed voxel: the one nearest `near` (default: the middle of the bounds), ties broken by the draw"""
    p = np.unique(np.asarray(pos, np.int64).reshape(-1, 3), axis=0)
    near = (p.min(0) + p.max(0)) // 2 if near is None else np.asarray(near, np.int64)
    dist = np.abs(p - near).sum(axis=1)
    best = np.flatnonzero(dist == dist.min())
    return tuple(int(v) for v in p[best[rng.integers(0, len(best))]])


def from_map(rng, m, t, box_min, box_max, share=3, within=None, extra=None, first=1.0):
    """A list made from a map and a box: a random 1 / share of the distinct source cells that the box's in-range cells pull, and for
    each a decoy one cell off on a random axis (a near miss, unless another cell pulls it).  within = (lo, hi): only voxels inside
    that box, whose two corners are listed too, so that the list's bounds are exactly it.  extra: positions listed as well.
    first: only what the first so many of the box's cells, in block order, pull (magnify lists all of that: its first blocks
    hit in every cell)."""
    cells = box_cells(box_min, box_max)
    _, s, ok = pulled(m, t, cells[:max(1, int(first * len(cells)))])
    s = np.unique(s[ok], axis=0)
    if within is not None:
        lo, hi = np.array(within[0], np.int64), np.array(within[1], np.int64)
        s = s[((s >= lo) & (s <= hi)).all(axis=1)]
    take = s[rng.random(len(s)) < 1.0 / share] if share else s[:0]
    if len(take) == 0 and len(s) and share:
        take = s[rng.integers(0, len(s), 1)]
    if first < 1.0:          # all of it but what the box's last cell pulls: the result is not the whole box; no decoys
        last = pulled(m, t, cells[-1:])[1][0]
        take = take[(take != last).any(axis=1)]
        assert len(take) >= 1
    step = np.zeros_like(take)
    step[np.arange(len(take)), rng.integers(0, 3, len(take))] = rng.choice((-1, 1), len(take))
    decoy = take + step
    parts = [take, decoy] if first == 1.0 else [take]
    if share == 0:                   # nothing the box pulls is listed: the neighbours of what it pulls are
        parts = [np.array([[v + 1 if v < T.HI else v - 1 for v in row] for row in s.tolist()], np.int64).reshape(-1, 3)]
    if within is not None:
        parts += [lo[None, :], hi[None, :]]
    if extra is not None:
        parts.append(np.asarray(extra, np.int64).reshape(-1, 3))
    cells = np.concatenate(parts)
    if within is not None:
        cells = cells[((cells >= lo) & (cells <= hi)).all(axis=1)]
    cells = cells[((cells >= T.LO) & (cells <= T.HI)).all(axis=1)]
    if len(cells) == 0:
        cells = np.zeros((1, 3), np.int64)
    return _listed(rng, cells)


# ---- boxes: the three block shapes ----------------------------------------------------------------------------------------------------
SHAPES = ("run", "rows", "slab")


def shaped(rng, shape):
    """extents whose blocks have the shape: a z run over 2 048 cells; rows with ey ez >= 2 048 and odd extents such as (5, 37, 61);
    slabs with ey ez < 2 048"""
    if shape == "run":
        return (int(rng.integers(1, 4)), int(rng.integers(1, 4)), 2049 + int(rng.integers(0, 250)))
    if shape == "rows":
        return (int(rng.integers(3, 8)), 37 + 2 * int(rng.integers(0, 6)), 59 + 2 * int(rng.integers(0, 5)))
    return (21 + 2 * int(rng.integers(0, 13)), 5 + 2 * int(rng.integers(0, 5)), 7 + 2 * int(rng.integers(0, 5)))


def placed(ext, centre):
    """the box of those extents around a centre, clipped at +-32768"""
    lo = [int(c) - e // 2 for c, e in zip(centre, ext)]
    return tuple(max(-32768, v) for v in lo), tuple(min(32768, v + e) for v, e in zip(lo, ext))


def middle_cell(box_min, box_max):
    return tuple((int(a) + int(b) - 1) // 2 for a, b in zip(box_min, box_max))


def diag(a):
    return [[int(a[0]), 0, 0], [0, int(a[1]), 0], [0, 0, int(a[2])]]


def random_rotation(rng):
    """a rotation from a uniformly drawn unit quaternion"""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ---- the map families: each -> [spec], a spec being a dict with m, box, the fixed list's name and, for from_map, t -------------------
# A spec's keys: m; box = (box_min, box_max); fixed = a name of FIXED; t = the offset of the from_map case (default: the middle
# cell pulls (0, 0, 0)) and, with exact_t, of the fixed case too; anchor = the cell whose pull of the list's middle voxel the
# fixed case's t is solved for (default: the middle cell); rest = solve_t's; share / first = from_map's; rigid = (rotation, pivot,
# translation) and near = (shape, axis, side, clearance) instead of m and t; rank, whole, wraps, empty and meta go to META.
META = {}


def _limits(rng):
    big = (T.M_LIMIT, T.M_LIMIT - 1)
    specs = []
    # rows of equal-signed +-2^24 with t against the row's sign at +-2^40, in a 24^3 box where the sums cancel
    for k, (signs, side) in enumerate(zip(((1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, -1), (1, 1, -1), (-1, -1, -1)), (1, -1, 1, -1, 1, -1))):
        e = [big[(k + i) % 2] if k >= 2 else T.M_LIMIT for i in range(3)]
        m = [[signs[i] * e[i]] * 3 for i in range(3)]
        tl = T.T_LIMIT - (1 if k in (3, 4) else 0)
        centre = (21845,) * 3 if side > 0 else (-21846,) * 3
        box = placed((24, 24, 24), centre)
        # the fixed list: a cell of the box whose sum of 2 d + 1 is 131071 in size, one less than what passes 2^40
        anchor = (21845, 21845, 21844) if side > 0 else (-21846, -21846, -21845)
        specs.append(dict(m=m, t=[-signs[i] * side * tl for i in range(3)], box=box, fixed="blob", anchor=anchor))
    # one row at the limits with mixed signs, the others rotation-sized: rank 3.  The box lies where the row's sum cancels its t.
    for k, (signs, shape, clip) in enumerate((((1, -1, 1), "run", False), ((-1, 1, 1), "rows", False), ((1, 1, -1), "slab", False), ((1, -1, 1), "rows", True),
                                              ((-1, -1, 1), "run", False))):
        r = np.rint(random_rotation(rng) * ONE).astype(np.int64).tolist()
        row = k % 3
        ext = shaped(rng, shape)
        for j in range(3):
            r[row][j] = signs[j] * big[(k + j) % 2]
        side = 1 if k % 2 == 0 else -1
        centre = [21845 if signs[j] * side > 0 else -21846 for j in range(3)]          # the signed sum of 2 d + 1 is 131073 side
        if clip or shape == "run":          # 2 d + 1 = +-65535, +-65535, +-3: the box is clipped at 32768 and at -32768
            centre = [32767 if signs[j] * side > 0 else -32768 for j in range(3)]
            centre[2] = 1 if signs[2] * side > 0 else -2
        if shape == "run":          # a z run of 2 048 cells at 256 cells a cell leaves the range: the row's z entry is rotation-sized
            r[row][2] = signs[2] * 3 * ONE // 4
            centre[2] = 0
        box = placed(ext, centre)
        t = solve_t([[0, 0, 0] if i == row else r[i] for i in range(3)], middle_cell(*box), (0, 0, 0))
        t[row] = -side * (T.T_LIMIT - k % 2)
        specs.append(dict(m=r, t=t, box=box, fixed="blob"))
    return specs


def _magnify(rng):
    specs = []
    for k in range(12):
        a = [int(rng.choice((-1, 1))) * int(rng.integers(1 << 10, (1 << 15) + 1)) for _ in range(3)]
        shape = SHAPES[k % 3]
        if shape == "run":
            a[2] = int(rng.choice((-1, 1))) * int(rng.integers(1 << 10, 1 << 12))
        ext = shaped(rng, shape)
        centre = (32760, -32760, 5) if k == 4 else tuple(rng.integers(-50, 50, 3).tolist())
        specs.append(dict(m=diag(a), box=placed(ext, centre), fixed=("clustered", "blob")[k % 2], share=1, first=0.6))
    return specs


def _minify(rng):
    specs = []
    for k in range(12):
        if k % 2 == 0:
            m = diag([int(rng.choice((-1, 1))) * int(rng.integers(1 << 18, (1 << 24) + 1)) for _ in range(3)])
        else:
            m = (rng.choice((-1, 1), (3, 3)) * rng.integers(1 << 16, (1 << 22) + 1, (3, 3))).tolist()
        shape = SHAPES[k % 3]
        if shape == "run":          # a run of 2 048 cells stays inside the range at up to 8 cells a cell
            for i in range(3):
                m[i][2] = int(np.sign(m[i][2])) * int(rng.integers(1 << 16, 1 << 19)) if m[i][2] else 0
        ext = shaped(rng, shape)
        centre = (-32765, 32760, -32764) if k == 5 else tuple(rng.integers(-40, 40, 3).tolist())
        specs.append(dict(m=m, box=placed(ext, centre), fixed=("far", "clustered", "blob")[k % 3 if k < 9 else 0]))
    return specs


def _shear(rng):
    specs = []
    for k in range(12):
        m = T.identity()[0]
        for i in range(3):
            for j in range(3):
                if i != j and rng.random() < 0.7:
                    m[i][j] = int(rng.integers(-2 * ONE, 2 * ONE + 1))
        m[k % 3][(k + 1) % 3] = (2 * ONE, -2 * ONE)[k // 3 % 2]       # the greatest shear, in either sign
        shape = SHAPES[k % 3]
        centre = (32750, 20, -32760) if k == 7 else tuple(rng.integers(-30, 30, 3).tolist())
        specs.append(dict(m=m, box=placed(shaped(rng, shape), centre), fixed=("plane", "blob", "line")[k % 3 if k < 6 else k % 2]))
    return specs


def _singular(rng):
    specs = []
    zero = [[0, 0, 0] for _ in range(3)]
    # rank 0: every cell pulls the one voxel t names: the whole box or nothing
    specs.append(dict(m=zero, box=placed((9, 40, 57), (3, -2, 1)), fixed="blob", rank=0, whole=True))
    specs.append(dict(m=zero, box=placed((2, 2, 2100), (0, 0, 0)), fixed="line", rank=0, whole=True))
    specs.append(dict(m=zero, box=placed((31, 9, 11), (32760, 32760, -32760)), fixed="far", rank=0, whole=False, share=0, nudge=True))
    # rank 2: projections along an axis (a whole line of cells pulls one voxel) and along the diagonal (1, 1, 1)
    for k, axis in enumerate((0, 1, 2, 2)):
        m = diag([(ONE, -ONE)[(k + i) % 2] for i in range(3)])
        m[axis][axis] = 0
        specs.append(dict(m=m, box=placed(shaped(rng, SHAPES[k % 3]), rng.integers(-8, 8, 3).tolist()), fixed=("blob", "plane")[k % 2], rank=2))
    for k in range(2):
        s = (ONE, ONE // 2)[k]
        m = [[s, -s, 0], [0, s, -s], [0, 0, 0]]
        specs.append(dict(m=m, box=placed(shaped(rng, SHAPES[1 + k]), rng.integers(-8, 8, 3).tolist()), fixed="blob", rank=2))
    # rank 1: every row a multiple of one
    for k in range(3):
        v = [int(x) for x in rng.integers(-ONE, ONE + 1, 3)]
        u = (1, -2, 1) if k else (1, 0, 0)
        m = [[u[i] * v[j] for j in range(3)] for i in range(3)]
        if SHAPES[k] == "run":
            for i in range(3):
                m[i][2] = u[i] * int(rng.integers(-ONE // 64, ONE // 64))
        specs.append(dict(m=m, box=placed(shaped(rng, SHAPES[k]), rng.integers(-8, 8, 3).tolist()), fixed=("blob", "line", "blob")[k], rank=1))
    return specs


def mirrors():
    """The 24 signed permutation matrices of determinant -1."""
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            r = [[signs[i] if perm[i] == j else 0 for j in range(3)] for i in range(3)]
            if round(float(np.linalg.det(np.array(r, np.float64)))) == -1:
                out.append(r)
    assert len(out) == 24
    return out


def _mirror(rng):
    specs = []
    for k, r in enumerate(mirrors()):
        twice_pivot = tuple(2 * int(v) + k % 2 for v in rng.integers(-6, 7, 3))        # all integers or all half-integers
        if k == 3:              # far out: the image lies at a corner of the range and its box is clipped
            twice_pivot = (32757, -32759, 32755)
        m, t = T.rotation_pull(r, twice_pivot)
        p = small_blob()[0].astype(np.int64)
        image = ((2 * p + 1 - np.array(twice_pivot)) @ np.array(r).T + np.array(twice_pivot) - 1) // 2
        if k % 3 == 0:          # the whole image of the list and two cells more: every voxel comes back
            box = tuple(max(-32768, int(v) - 2) for v in image.min(0)), tuple(min(32768, int(v) + 3) for v in image.max(0))
        else:                   # a box that cuts it
            centre = (image.min(0) + image.max(0)) // 2 + rng.integers(-3, 4, 3)
            box = placed(shaped(rng, SHAPES[k % 3 - 1] if k != 7 else "slab"), centre.tolist())
        specs.append(dict(m=m, t=t, box=box, fixed="small_blob", exact_t=True, meta=dict(r=r, twice_pivot=twice_pivot)))
    return specs


def _ties(rng):
    specs = []
    for k in range(13):
        if k % 2 == 0:          # multiples of 65536 with t a multiple of 32768
            m = (rng.integers(-2, 3, (3, 3)) * ONE).tolist()
            for i in range(3):
                m[i][i] = int(rng.choice((-1, 1))) * ONE
        else:                   # odd multiples of 32768
            m = ((2 * rng.integers(-2, 2, (3, 3)) + 1) * (ONE // 2) * (rng.random((3, 3)) < 0.6)).tolist()
            for i in range(3):
                m[i][i] = int(rng.choice((-3, -1, 1, 3))) * (ONE // 2)
        shape = SHAPES[k % 3]
        if shape == "run":
            for i in range(2):
                m[i][2] = 0
        ext = tuple(max(2, e) for e in shaped(rng, shape))
        box = placed(ext, (0, 0, 0) if k < 12 else (-32765, -32760, -32766))        # across 0 on every axis; the last is clipped at a corner
        t = [int(v) * (ONE // 2) for v in rng.integers(-8, 9, 3)]
        specs.append(dict(m=m, t=t, box=box, fixed=("blob", "plane")[1 if shape == "run" else 0], rest=lambda x: x % ONE))
    return specs


def _past_range(rng):
    specs = []
    ident = T.identity()[0]
    # by 1 to 3 cells on one axis, at a corner: the cells past the end would wrap into the cube at the other end
    for k, (axis, end) in enumerate(itertools.product(range(3), (1, -1))):
        corner = [T.HI if (k >> j) & 1 else T.LO for j in range(3)]
        corner[axis] = T.HI if end > 0 else T.LO
        t = [0, 0, 0]
        t[axis] = end * ONE * (1 + k % 3)
        lo = [c - 7 if c > 0 else c for c in corner]
        box = tuple(lo), tuple(v + 8 for v in lo)
        specs.append(dict(m=ident, t=t, box=box, fixed="far", exact_t=True, wraps=16))
    # by exactly 2^16 cells (t = +-2^32) and by exactly 2^24 cells (t = +-2^40): every cell is past the range, and wrapped in 16 bits,
    # or with P held in 32 bits, it is the cell itself
    for k, (far_t, axis) in enumerate(itertools.product((1 << 32, T.T_LIMIT), range(3))):
        t = [0, 0, 0]
        t[axis] = far_t * (1 if k % 2 else -1)
        c = CORNERS[(3 * k + 1) % 8] if k % 3 else (0, 0, 0)
        ext = ((9, 13, 11), (2, 2, 2100), (5, 37, 61))[k % 3]
        lo = [32768 - e if v > 0 else -32768 if v < 0 else -(e // 2) for v, e in zip(c, ext)]          # the box holds the cube there
        box = tuple(lo), tuple(v + e for v, e in zip(lo, ext))
        specs.append(dict(m=ident, t=t, box=box, fixed="far", exact_t=True, wraps=32, empty=True))
    # a scale of 2 and of -2 about the origin passes the range from |d| = 16384 on
    for k, a in enumerate((2 * ONE, -2 * ONE)):
        m = diag((a, ONE, ONE))
        box = (16380, -32768, 32760), (16388, -32760, 32768)
        specs.append(dict(m=m, t=[0, 0, 0], box=box, fixed="far", exact_t=True, wraps=16))
    return specs


def _rigid(rng):
    specs = []
    pivots = [(0.0, 0.0, 0.0), (0.5, -3.5, 7.5), (-11.5, 4.5, 0.5), (6.0, -2.0, 9.0)]
    for c in CORNERS:
        near = np.array(c) - np.sign(c) * rng.integers(0, 16, 3)
        pivots.append(tuple((near + (0.5 if len(pivots) % 2 else 0.0)).tolist()))
    for k, pivot in enumerate(pivots):
        r = random_rotation(rng)
        shift = tuple((rng.integers(-9, 10, 3) + (0.25 * rng.integers(0, 4, 3))).tolist())
        if not any(shift):
            shift = (1.0, -2.0, 0.75)
        specs.append(dict(rigid=(r, pivot, shift), fixed="small_blob"))
    return specs


def _near_miss_specs(rng):
    """Diagonal maps — translations and anisotropic scales of either sign.  For each block shape, source axis, side and clearance
    (one cell short, on the edge, one cell inside) one case: t on that axis is solved with the cull's interval rule so that a
    block's interval ends there; on the other axes the block's middle pulls the middle of the source's bounds.  A draw is kept when
    the restatement confirms the clearance, no other axis drops the block (unless it is the one-inside case of a degenerate
    bounding box, where the other side of the same axis may) and the model's result is not empty."""
    specs = []
    n = 0
    for shape in SHAPES:
        for axis in range(3):
            for side in ("below", "above"):
                for clear in (1, 0, -1):
                    fixed = ("blob", "plane", "line")[n // 3 % 3]
                    pos, mrgb = FIXED[fixed]()
                    for attempt in range(200):
                        a = [ONE, ONE, ONE] if (n + attempt) % 4 == 0 else [int(rng.choice((ONE // 2, ONE, 3 * ONE // 2, 40000, 100003))) for _ in range(3)]
                        a = [int(rng.choice((-1, 1))) * v for v in a]
                        ext = {"run": (3, 2, 4150 + n), "rows": (3, 67, 63), "slab": (91, 7, 11)}[shape]
                        centre = rng.integers(-20, 20, 3).tolist()
                        if n % 9 == 4:          # at an edge of the range: the box is clipped on x and y, and t carries it back
                            centre[:2] = [32767, -32760]
                        spec = dict(m=diag(a), box=placed(ext, centre), fixed=fixed, near=(shape, axis, side, clear),
                                    pick=float(rng.random()))
                        t, b = _place_near(spec, *bounds(pos))
                        _, _, below, above = cull(Case("", pos, mrgb, spec["m"], t, *spec["box"]))[b]
                        mine = (below if side == "below" else above)[axis]
                        others = [v for i in range(3) for v, s in ((below[i], "below"), (above[i], "above")) if (i, s) != (axis, side)]
                        # a rows block spans the box on z and a slab block on y and z: one cell short there, every block is, and
                        # the case's claim is emptiness
                        spans = clear == 1 and axis >= {"run": 3, "rows": 2, "slab": 1}[shape]
                        if mine == clear and (clear == -1 or max(others) <= 0) and (spans or hits(pos, spec["m"], t, *spec["box"])):
                            if spans:
                                spec["empty"] = True
                            break
                    else:
                        raise AssertionError(("near_miss: no draw", shape, axis, side, clear))
                    specs.append(spec)
                    n += 1
    return specs


def _place_near(spec, src_lo, src_hi):
    """-> (t, block index) for a near_miss spec against a source's bounds."""
    shape, axis, side, clear = spec["near"]
    m, box = spec["m"], spec["box"]
    bl = blocks(*box)
    of_shape = [b for b, (s, _, _) in enumerate(bl) if s == shape]
    b = of_shape[int(spec["pick"] * len(of_shape))]
    _, lo, hi = bl[b]
    mid = tuple((lo[j] + hi[j]) // 2 for j in range(3))
    t = solve_t(m, mid, tuple((src_lo[j] + src_hi[j]) // 2 for j in range(3)))
    u, v = m[axis][axis] * (2 * lo[axis] + 1), m[axis][axis] * (2 * hi[axis] + 1)
    if side == "below":          # the interval's greatest s is src_lo - clear
        x, target = max(u, v), src_lo[axis] - clear
    else:                        # the interval's least s is src_hi + clear
        x, target = min(u, v), src_hi[axis] + clear
    t[axis] = -((x - (target << 17)) // 2)          # x + 2 t in {target 2^17, target 2^17 + 1}
    assert (x + 2 * t[axis]) >> 17 == target
    return t, b


SPECS = {"limits": _limits, "magnify": _magnify, "minify": _minify, "shear": _shear, "singular": _singular, "mirror": _mirror, "ties": _ties,
         "past_range": _past_range, "rigid": _rigid, "near_miss": _near_miss_specs}


@functools.lru_cache(maxsize=None)
def specs(fam):
    return tuple(SPECS[fam](_rng(2, FAMILIES.index(fam))))


@functools.lru_cache(maxsize=None)
def case(fam, kind, k):
    """-> case k of a family for a list kind, a Case.  META[case.name] holds what it carries beside the tuple."""
    from gpu_voxel_raytracer_amd import host as H          # rigid_pull and rigid_box are plain Python: no library is loaded
    assert fam in FAMILIES and kind in KINDS
    spec = specs(fam)[k]
    rng = _rng(3, FAMILIES.index(fam), KINDS.index(kind), k)
    name = f"{fam}[{k}] {kind} (seed {SEED})"
    meta = dict(spec.get("meta", {}), family=fam, kind=kind, index=k, fixed=spec["fixed"])
    for key in ("rank", "whole", "wraps", "empty", "near"):
        if key in spec:
            meta[key] = spec[key]
    if "rigid" in spec:
        r, pivot, shift = spec["rigid"]
        a = H.rigid_pull(r, pivot, shift)
        m, t = [list(row) for row in a.m], list(a.t)
        pos, mrgb = FIXED[spec["fixed"]]()
        moved = np.clip(pos.astype(np.int64) + np.floor(np.array(pivot)).astype(np.int64), T.LO, T.HI)        # the list lies about the pivot
        pos = moved.astype(np.int16)
        src_lo, src_hi = bounds(pos)
        box = H.rigid_box(src_lo, src_hi, r, pivot, shift)
        if kind == "from_map":
            pos, mrgb = from_map(rng, m, t, *box, within=(src_lo, src_hi))
        meta.update(rotation=r, pivot=pivot, shift=shift)
    elif "near" in spec:
        m, box = spec["m"], spec["box"]
        pos, mrgb = FIXED[spec["fixed"]]()
        src_lo, src_hi = bounds(pos)
        t, meta["block"] = _place_near(spec, src_lo, src_hi)
        if kind == "from_map":
            pos, mrgb = from_map(rng, m, t, *box, within=(src_lo, src_hi))
    else:
        m, box = spec["m"], spec["box"]
        if kind == "from_map" or spec.get("exact_t"):
            t = spec["t"] if "t" in spec else solve_t(m, middle_cell(*box), (0, 0, 0))
        if kind == "from_map":
            extra = far()[0] if fam == "past_range" else None
            pos, mrgb = from_map(rng, m, t, *box, share=spec.get("share", 3), extra=extra, first=spec.get("first", 1.0))
        else:
            pos, mrgb = FIXED[spec["fixed"]]()
            if not spec.get("exact_t"):
                t = None
                for attempt in range(50):          # a draw whose t would pass 2^40 is redrawn
                    cell = spec.get("anchor") if attempt == 0 and "anchor" in spec else \
                        middle_cell(*box) if attempt == 0 else tuple(int(rng.integers(a, b)) for a, b in zip(*box))
                    voxel = middle_voxel(pos, rng, near=NEAR.get(spec["fixed"]))
                    if spec.get("nudge"):          # rank 0, nothing: the cell beside a voxel that is not listed
                        listed = set(map(tuple, pos.tolist()))
                        voxel = next(v for v in ((voxel[0] + d, voxel[1], voxel[2]) for d in range(1, 99)) if v not in listed)
                    t = solve_t(m, cell, voxel, spec.get("rest"))
                    if t is not None:
                        break
                assert t is not None, name
    T.check_map(m, t)
    ext = extents(*box)
    assert 0 < ext[0] * ext[1] * ext[2] <= MAX_BOX, (name, ext)
    assert all(-32768 <= v <= 32768 for v in box[0] + box[1]), name
    META[name] = meta
    return Case(name, pos, mrgb, [list(map(int, row)) for row in m], [int(v) for v in t], tuple(box[0]), tuple(box[1]))


def count(fam):
    return len(specs(fam))


def family(fam, kind):
    """-> the family's cases for a list kind, a tuple of Case"""
    return tuple(case(fam, kind, k) for k in range(count(fam)))


# the cases of a family that one GPU test takes (tests/test_gpu_transform_families.py): sized so that a test, the model's walk
# included, stays under the longest case of tests/test_gpu_transform.py
PART = {"mirror": 2, "near_miss": 6, "rigid": 3, "singular": 4}


def parts(fam):
    """-> [range of case indices] per part"""
    n, step = count(fam), PART.get(fam, 6)
    return [range(a, min(a + step, n)) for a in range(0, n, step)]


@functools.lru_cache(maxsize=None)
def expected(fam, kind, index):
    """The model's result of a case: transform_np's walk of its whole box -> (pos int16 [k,3], mrgb uint8 [k,4]), shared and never
    written."""
    c = case(fam, kind, index)
    got = T.transform_np(c.pos, c.mrgb, c.m, c.t, c.box_min, c.box_max)
    for a in got:
        a.setflags(write=False)
    return got


def cells_of(case):
    ext = extents(case.box_min, case.box_max)
    return ext[0] * ext[1] * ext[2]
