"""Voxel lists that the combiner, the morphology and the mesher dislike, by family, and the models' result of each (no GPU, no
library).

A family is a tuple of cases `Case(name, pos int16 [n,3], mrgb uint8 [n,4])`; the name carries family, index and seed.  Except for
the bars of `long_runs` a list is shuffled and about 5 % of its positions are listed again with other bytes (the last entry wins).
The generators are seeded and deterministic; the expected results are the brute-force models' (morph_model, mesh_model,
setops_model), cached so that a case computes each once (`morphed`, `meshed`, `combined`) and never written.
tests/test_list_families_cpu.py checks with the models alone that each family is what it claims;
tests/test_gpu_list_families.py sends them through the device.

The module restates two things in numpy, for CLASSIFYING cases only (no byte of an expected result comes from them): the
depth-15 path key (`path_keys`, transform_families') and where in the sorted faces the runs along a bar begin (`run_base`).

What could not be built as the families were first described, and why:
* `vertex_counts` has no list of 7, 9 or 17 vertices.  A mesh that is not empty has at least the 8 corners of one voxel; the
  counts that unions of far-apart pieces reach are sums of 8 (a voxel), 14 (an edge-touching pair), 15 (a corner-touching pair),
  19 and 23 (three and four voxels around one corner) and 4 L + 4 (a bar), and the least sum that is 1 mod 4 is 14 + 15 = 29.
  The search (`_pieces`, `_solve`) keeps only pieces without two face-adjacent voxels off a bar, so that every quad off a bar is
  one face and the count is the same in both modes, with and without bytes.  k = 3 gives 8 alone and k = 4 gives 15 and 16.
  7 and 9 cannot be: one voxel has 8 vertices and two or more have 12 at least.  17 was searched for beyond these pieces, in
  both modes (RUNS drops the vertices inside a long quad): no union of up to 6 voxels of a 3 x 3 x 2 block has 17 in either.
* a strictly periodic colouring of a bar cannot put a head on both sides of a block when the period is even or near 2 048: the
  heads of one run stand at one residue.  A bar of `long_runs` therefore has its period in two phases: the first half's
  boundaries are placed so that a sorted face at a multiple of 2 048 begins a quad, the second half's so that one at a multiple
  of 2 048 less 1 does (`period_targets`).
* each period runs on one axis (period i on axis i mod 3), not on all three: the mesher's model takes 5.6 s for one coloured
  bar in both modes, and 24 bars would be two minutes of every later run of the suite.  Every axis carries the full one-colour
  bar, the bit-7 bar and at least two periods, one of them of 2 047 to 2 049 cells.  The mutations of the head test and of
  `before` (tests/test_gpu_list_families.py's table) are noticed by the bars of every axis."""
import functools
import itertools
from typing import NamedTuple

import numpy as np

import mesh_model as MM
import morph_model as M
import setops_model as S
from transform_families import path_keys
from transform_model import HI, LO

SEED = 2711
SPAN = 2048                         # morph_rule.h: kMorphSpan, setops_rule.h: kSetopSpan — the entries of a block
FAMILIES = ("seams", "range_faces", "far", "sizes", "vertex_counts", "long_runs", "checker")
MAX_LIST = 20_000                   # entries, the full bars excepted
BAR = 65536
MORPH_WIDE = 5000                   # the most distinct cells that go through the morphology's model at connectivity 18 or 26

# ---- what the generators give with SEED (tests/test_list_families_cpu.py asserts it) -----------------------------------------------
# A claim that is a count or a share has a floor: half of what these generators give, rounded down to two digits
# (mesh_families.FLOOR's convention).  The claims that hold exactly are in the CPU file.
FLOOR = {
    ("seams", "occupancy of a cluster's 4^3 cells"): 0.23,                               # measured 0.478 (clusters overlap near the origin)
    ("seams", "listed pairs one step apart whose step carries or borrows 6 to 14 bits"): 9500,      # measured 19 138
    ("seams", "distinct patterns of bits 6 to 14 of u, over the three axes"): 16,        # measured 32 (2 in the hand-written lists)
    ("range_faces", "occupancy of a patch's 3^3 cells"): 0.26,                           # measured 0.537 to 0.587
    ("range_faces", "listed voxels with a neighbour outside the range"): 320,            # measured 646
    ("far", "share of voxels without a listed neighbour at connectivity 26"): 0.40,      # measured 0.805, 0.807 and 0.803
    ("far", "distinct patterns of bits 6 to 14 of u on one axis"): 150,                  # measured 511, 512 and 307 (far[2], 600 cells) of 512
    ("sizes", "share of entries that list a position again"): 0.022,                     # measured 0.0454
    ("long_runs", "run heads at distinct item positions of a thread, period 7"): 4,      # measured 8 of 8
    ("checker", "entries of the longest group of equal corner keys"): 6,                 # measured 12
    ("checker", "groups of equal corner keys that straddle a block boundary"): 17,       # measured 34 of 34 boundaries, in each list
}


class Case(NamedTuple):
    name: str
    pos: np.ndarray
    mrgb: np.ndarray


def _rng(*where):
    return np.random.default_rng([SEED, *where])


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _name(fam, k):
    return f"{fam}[{k}] (seed {SEED})"


def _listed(rng, cells):
    """distinct cells -> (pos, mrgb): random bytes, 5 % of the positions listed again with other bytes, shuffled"""
    cells = np.unique(np.asarray(cells, np.int64).reshape(-1, 3), axis=0)
    assert len(cells) and cells.min() >= LO and cells.max() <= HI
    cells = np.concatenate([cells, cells[rng.integers(0, len(cells), max(1, len(cells) // 20))]])
    cells = cells[rng.permutation(len(cells))]
    return cells.astype(np.int16), rng.integers(0, 256, (len(cells), 4)).astype(np.uint8)


def _case(fam, k, pos, mrgb, limit=MAX_LIST):
    assert len(pos) <= limit and len(pos) == len(mrgb), (fam, k, len(pos))
    return Case(_name(fam, k), *_frozen(np.ascontiguousarray(pos, np.int16), np.ascontiguousarray(mrgb, np.uint8)))


def distinct(pos):
    return np.unique(np.asarray(pos, np.int64).reshape(-1, 3), axis=0)


def _block(side):
    g = np.arange(side)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


# ---- seams: 4^3 clusters centred on points of {0, +-2^k} ------------------------------------------------------------------------------
SEAM_VALUES = (0,) + tuple(s << k for k in range(15) for s in (1, -1))
SEAM_CASES = 4
SEAM_FORCED = ((0, 0, 0), (-1, -1, -1), (-1, 0, 0), (0, -1, 0), (0, 0, -1))


@functools.lru_cache(maxsize=None)
def seam_centres():
    """Per k in 0 .. 14 and sign the centres (c, c, c), (c, c, r), (c, r, c) and (r, c, c), c = +-2^k and r another value of the set
    (a cluster there holds the diagonal pair across c on three and on two axes), the origin, and 100 centres drawn from the set."""
    rng = _rng(1, 0)
    out = [(0, 0, 0)]
    for k in range(15):
        for s in (1, -1):
            c = s << k
            r = [int(rng.choice(SEAM_VALUES)) for _ in range(3)]
            out += [(c, c, c), (c, c, r[0]), (c, r[1], c), (r[2], c, c)]
    out += [tuple(int(v) for v in rng.choice(SEAM_VALUES, 3)) for _ in range(100)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def seams():
    """Cells c - 2 .. c + 1 per axis around each centre at occupancy about 0.5.  Five cells are always listed, because the exact
    claims rest on them: the centre c, c - (1, 1, 1), and c less one on each single axis — steps across the centre on one, two
    and three axes.  Centre i goes to case i mod 4."""
    cube = _block(4) - 2
    cases = []
    for k in range(SEAM_CASES):
        rng = _rng(1, 1, k)
        parts = []
        for centre in seam_centres()[k::SEAM_CASES]:
            at = cube[rng.random(len(cube)) < 0.5 - 5 / 64]
            parts.append(np.concatenate([at, SEAM_FORCED]) + np.array(centre))
        cases.append(_case("seams", k, *_listed(rng, np.concatenate(parts))))
    return tuple(cases)


# ---- range_faces: 3^3 patches against the faces, edges and corners of the int16 cube -----------------------------------------------
DIRECTIONS26 = tuple(o for o in itertools.product((-1, 0, 1), repeat=3) if any(o))
RANGE_CASES = 3


@functools.lru_cache(maxsize=None)
def range_faces():
    """Per case and per direction of the 26 one patch at occupancy about 0.6, pushed against the range where the direction is
    nonzero and drawn from [-30000, 30000] where it is zero.  The patch's outermost cell in its direction and the cell one step
    back are always listed."""
    cube = _block(3)
    cases = []
    for k in range(RANGE_CASES):
        rng = _rng(2, k)
        parts = []
        for d in DIRECTIONS26:
            origin = np.array([HI - 2 if v > 0 else LO if v < 0 else int(rng.integers(-30000, 30001)) for v in d])
            outer = np.array([2 if v > 0 else 0 if v < 0 else 1 for v in d])
            at = cube[rng.random(len(cube)) < 0.6 - 2 / 27]
            parts.append(np.concatenate([at, [outer, outer - np.array(d)]]) + origin)
        cases.append(_case("range_faces", k, *_listed(rng, np.concatenate(parts))))
    return tuple(cases)


# ---- far: uniform over the whole range ---------------------------------------------------------------------------------------------------
FAR_SIZES = (MORPH_WIDE, 16385, 600)


@functools.lru_cache(maxsize=None)
def far():
    """far[0]: 5 000 distinct cells, far[1]: 16 385, far[2]: 600 (small enough for two steps of the morphology's model) — nine
    tenths uniform over the range, a tenth one step (of the 26) from one of them, so that almost all are isolated and the rest are
    not."""
    cases = []
    for k, m in enumerate(FAR_SIZES):
        rng = _rng(3, k)
        cells = distinct(rng.integers(LO, HI + 1, (m - m // 10, 3)))
        while len(cells) < m:
            short = m - len(cells)
            more = cells[rng.integers(0, len(cells), short)] + np.array(DIRECTIONS26)[rng.integers(0, 26, short)]
            cells = distinct(np.concatenate([cells, np.clip(more, LO, HI)]))
        cases.append(_case("far", k, *_listed(rng, cells)))
    return tuple(cases)


# ---- sizes: distinct counts at the walk's edges ----------------------------------------------------------------------------------------
def size_counts():
    """m = 2^k - 1, 2^k, 2^k + 1 for k = 1 .. 14 and 2048 j - 1, 2048 j, 2048 j + 1 for j = 1 .. 4, ascending, each once"""
    out = {(1 << k) + e for k in range(1, 15) for e in (-1, 0, 1)} | {SPAN * j + e for j in range(1, 5) for e in (-1, 0, 1)}
    return tuple(sorted(out))


@functools.lru_cache(maxsize=None)
def sizes():
    """Per count m a list of m distinct cells drawn from the box [-h, h)^3 around the origin that holds 8 m cells at least (one in
    eight is listed: sparse, and the keys straddle the origin's seam on every axis); n > m through the duplicates."""
    cases = []
    for k, m in enumerate(size_counts()):
        rng = _rng(4, k)
        h = 2
        while (2 * h) ** 3 < 8 * m:
            h += 1
        flat = np.sort(rng.permutation((2 * h) ** 3)[:m])
        cells = np.stack([flat // (4 * h * h), flat // (2 * h) % (2 * h), flat % (2 * h)], -1) - h
        cases.append(_case("sizes", k, *_listed(rng, cells)))
    return tuple(cases)


# ---- vertex_counts: meshes of 2^k - 1, 2^k, 2^k + 1 vertices ---------------------------------------------------------------------------
def _vertices(cells, mode=MM.FACES, mrgb=None):
    return len(MM.mesh(np.asarray(cells, np.int16).reshape(-1, 3), mrgb, mode)[0])


@functools.lru_cache(maxsize=None)
def _pieces():
    """The search over small unions: every subset of a 2^3 block without two face-adjacent voxels -> {vertices: cells}, the first
    found per count.  Such a piece's quads are single faces in both modes."""
    block = _block(2)
    found = {}
    for bits in range(1, 256):
        cells = block[[i for i in range(8) if bits >> i & 1]]
        if any(np.abs(a - b).sum() == 1 for a, b in itertools.combinations(cells, 2)):
            continue
        found.setdefault(_vertices(cells), cells)
    return found


def _solve(target):
    """-> (pieces' vertex counts, bar length or 0) whose sum is `target`, or None: at most three pieces and one bar of 4 L + 4"""
    counts = sorted(_pieces())
    for n in range(4):
        for combo in itertools.combinations_with_replacement(counts, n):
            rest = target - sum(combo)
            if rest == 0 or (rest >= 8 and rest % 4 == 0):
                return combo, (rest // 4 - 1 if rest else 0)
    return None


def vertex_targets():
    return tuple(sorted({(1 << k) + e for k in range(3, 14) for e in (-1, 0, 1)}))


UNREACHABLE = (7, 9, 17)            # the module's docstring


def vertex_reachable():
    """The targets that have a list: vertex_counts()[k] has vertex_reachable()[k] vertices."""
    return tuple(t for t in vertex_targets() if t not in UNREACHABLE)


@functools.lru_cache(maxsize=None)
def vertex_counts():
    """Per reachable target (vertex_reachable, in its order) one list: the pieces 8 cells apart along y, the bar along z (x, y for
    the next targets) 8 cells off."""
    cases = []
    for k, target in enumerate(vertex_reachable()):
        rng = _rng(5, k)
        combo, length = _solve(target)
        parts = [_pieces()[c] + np.array([0, 8 * i, 0]) for i, c in enumerate(combo)]
        if length:
            bar = np.zeros((length, 3), np.int64)
            bar[:, (2, 0, 1)[k % 3]] = np.arange(length) - length // 2
            parts.append(bar + np.array([-8, -8, -8]) * np.array([(1, 1, 0), (0, 1, 1), (1, 0, 1)][k % 3]))
        cases.append(_case("vertex_counts", k, *_listed(rng, np.concatenate(parts))))
    return tuple(cases)


# ---- long_runs: the full bars -------------------------------------------------------------------------------------------------------------
PERIODS = (1, 2, 7, 8, 9, 2047, 2048, 2049)
PALETTE = np.array([[1, 200, 10, 10], [2, 10, 200, 10], [3, 10, 10, 200]], np.uint8)
THROUGH = (5, -7, 3)               # the bars' coordinates on the other two axes (mesh_model.bar's)


def run_base(axis):
    """The index among a full bar's sorted faces of the first face of direction (axis + 1) % 3, whose 65 536 faces run along the
    bar in its order: the directions before it have 65 536 faces each, or 1 where their normal is the bar's axis.  Classification
    only; the CPU file holds it against the model."""
    d = (axis + 1) % 3
    return sum(1 if MM.axis_of(e) == axis else BAR for e in range(d))


def period_targets(axis):
    """The two sorted faces that a coloured bar makes heads: the first of a block (a multiple of 2 048) among the first half's
    faces of the run direction, and the last of a block among the second half's."""
    base = run_base(axis)
    first = (base // SPAN + 1) * SPAN
    second = (base + BAR // 2) // SPAN * SPAN + 2 * SPAN - 1
    return first, second


def period_boundaries(axis, period):
    """The cells (indices along the bar) at which the colour changes: period apart in each half, the first half's placed so that
    period_targets' first face begins a quad, the second half's so that its second does."""
    base = run_base(axis)
    first, second = (t - base for t in period_targets(axis))
    assert 0 < first < BAR // 2 < second < BAR
    return np.concatenate([np.arange(first % period or period, BAR // 2, period), np.arange(BAR // 2 + ((second - BAR // 2) % period or period), BAR, period)])


def bar_cells(axis):
    p = np.tile(np.array(THROUGH, np.int16), (BAR, 1))
    p[:, axis] = np.arange(LO, HI + 1)
    return p


LONG_KINDS = tuple([("one colour", a, None) for a in range(3)] + [("period", i % 3, p) for i, p in enumerate(PERIODS)] + [("bit 7", a, None) for a in range(3)])


@functools.lru_cache(maxsize=None)
def long_runs():
    """LONG_KINDS[k] = (kind, axis, period) of case k.  In order along the bar, nothing listed twice."""
    cases = []
    for k, (kind, axis, period) in enumerate(LONG_KINDS):
        rng = _rng(6, k)
        if kind == "one colour":
            mrgb = MM.one_colour(BAR)
        elif kind == "period":
            colour = np.zeros(BAR, np.int64)
            colour[period_boundaries(axis, period)] = 1
            mrgb = PALETTE[np.cumsum(colour) % 3]
        else:
            mrgb = MM.one_colour(BAR)
            mrgb[:, 0] |= (rng.integers(0, 2, BAR) << 7).astype(np.uint8)
        cases.append(_case("long_runs", k, bar_cells(axis), mrgb, limit=BAR))
    return tuple(cases)


PIECE = (8, BAR // 2, BAR // 2 + 2 * SPAN + 1)      # case, first cell, end: 4 097 cells of the bar of period 2 047, from its middle on


@functools.lru_cache(maxsize=None)
def bar_piece():
    """A piece of a full bar short enough for two steps of the morphology's model (the second works on five times the cells): the
    colour changes three times inside it."""
    k, lo, hi = PIECE
    bar = long_runs()[k]
    return Case(f"long_runs[{k}][{lo}:{hi}] (seed {SEED})", *_frozen(bar.pos[lo:hi].copy(), bar.mrgb[lo:hi].copy()))


# ---- checker ---------------------------------------------------------------------------------------------------------------------------
CHECKER_SIDE, CHECKER_AT = 18, -9


@functools.lru_cache(maxsize=None)
def checker():
    """The cells of even, and of odd, coordinate sum of the block [-9, 9)^3."""
    block = _block(CHECKER_SIDE) + CHECKER_AT
    cases = []
    for k in range(2):
        rng = _rng(7, k)
        cases.append(_case("checker", k, *_listed(rng, block[block.sum(axis=1) % 2 == k])))
    return tuple(cases)


GENERATORS = {"seams": seams, "range_faces": range_faces, "far": far, "sizes": sizes, "vertex_counts": vertex_counts, "long_runs": long_runs,
              "checker": checker}


def family(fam):
    return GENERATORS[fam]()


def case(fam, k):
    return family(fam)[k]


# ---- pairs, for the combiner ---------------------------------------------------------------------------------------------------------------
class Pair(NamedTuple):
    name: str
    a: tuple            # (pos, mrgb)
    b: tuple
    meta: dict


def by_key(pos, mrgb):
    """-> (keys ascending, pos, mrgb) of a list's distinct positions with the bytes of each one's last entry (bit 7 as listed)"""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    keys = path_keys(pos)
    order = np.argsort(keys, kind="stable")
    last = np.append(keys[order][1:] != keys[order][:-1], True)
    at = order[last]
    return keys[at], pos[at].astype(np.int16), np.asarray(mrgb)[at]


def merged_items(a_pos, b_pos):
    """The merged sequence of the two lists' distinct keys, A's item first on equal keys -> [(key, 0 for A or 1 for B)]"""
    ka, kb = (np.unique(path_keys(np.asarray(p, np.int64).reshape(-1, 3))) for p in (a_pos, b_pos))
    return sorted([(int(k), 0) for k in ka] + [(int(k), 1) for k in kb])


@functools.lru_cache(maxsize=None)
def pairs():
    out = []

    def add(kind, a, b, **meta):
        k = len(out)
        name = f"pairs[{k}] {kind} (seed {SEED})"
        assert max(len(a[0]), len(b[0])) <= MAX_LIST
        out.append(Pair(name, _frozen(*(np.ascontiguousarray(v) for v in a)), _frozen(*(np.ascontiguousarray(v) for v in b)), dict(meta, kind=kind)))

    # B = A moved one cell across a seam, per axis
    for axis in range(3):
        rng = _rng(8, 0, axis)
        a = seams()[axis]
        step = np.zeros(3, np.int64)
        step[axis] = (1, -1, 1)[axis]
        add("moved", (a.pos, a.mrgb), ((a.pos.astype(np.int64) + step).astype(np.int16), rng.integers(0, 256, a.mrgb.shape).astype(np.uint8)), axis=axis)
    # B a random subset, and a random superset, of A: half of B's entries keep A's bytes
    for k, kind in enumerate(("subset", "superset")):
        rng = _rng(8, 1, k)
        a = far()[1] if kind == "subset" else range_faces()[0]
        _, pos, mrgb = by_key(a.pos, a.mrgb)
        if kind == "subset":
            keep = rng.random(len(pos)) < 0.5
            b_pos, b_mrgb = pos[keep], mrgb[keep].copy()
        else:
            extra = np.clip(pos[rng.integers(0, len(pos), len(pos))].astype(np.int64) + rng.integers(-2, 3, (len(pos), 3)), LO, HI).astype(np.int16)
            b_pos, b_mrgb = np.concatenate([pos, extra]), np.concatenate([mrgb, rng.integers(0, 256, (len(extra), 4)).astype(np.uint8)])
        other = rng.random(len(b_pos)) < 0.5
        b_mrgb[other] = rng.integers(0, 256, (int(other.sum()), 4)).astype(np.uint8)
        order = rng.permutation(len(b_pos))
        add(kind, (a.pos, a.mrgb), (b_pos[order], b_mrgb[order]))
    # B = A with bytes that differ only in bit 7
    rng = _rng(8, 2)
    a = checker()[0]
    b_mrgb = a.mrgb.copy()
    b_mrgb[:, 0] ^= (rng.integers(0, 2, len(b_mrgb)) << 7).astype(np.uint8)
    add("bit 7", (a.pos, a.mrgb), (a.pos, b_mrgb))
    # B = A with one byte changed at the key of merged item 2048 j - 1 or 2048 j.  A's keys are B's and one voxel that sorts first:
    # the equal pairs lie at merged items (2 i + 1, 2 i + 2), one across every block boundary (test_setops_cpu.straddle_lists).
    # "at" = 2048 j - 1: that pair's key, A's item before the boundary and B's behind it.  "at" = 2048 j: the lists without the
    # extra voxel, the pairs at (2 i, 2 i + 1): A's item opens block j.
    base = next(c for c in sizes() if len(distinct(c.pos)) == 4 * SPAN + 1)
    _, pos, mrgb = by_key(base.pos, base.mrgb)
    for j in range(1, 5):
        for at in (SPAN * j - 1, SPAN * j):
            rng = _rng(8, 3, j, at)
            first = 0 if at % 2 else 1
            a_pos, a_mrgb = pos[first:], mrgb[first:]
            b_pos, b_mrgb = pos[1:], mrgb[1:].copy()
            i = (at - 1) // 2 if at % 2 else at // 2               # the index in B of the key at merged item `at`
            b_mrgb[i, int(rng.integers(1, 4))] ^= 1 << int(rng.integers(0, 8))
            oa, ob = rng.permutation(len(a_pos)), rng.permutation(len(b_pos))
            add("one byte", (a_pos[oa], a_mrgb[oa]), (b_pos[ob], b_mrgb[ob]), at=at, key=int(path_keys(b_pos[i:i + 1].astype(np.int64))[0]))
    # A and B alternating in runs of 1 .. 9 keys of one list; a twentieth of the keys in both
    for k, src in enumerate((far()[0], seams()[3])):
        rng = _rng(8, 4, k)
        _, pos, mrgb = by_key(src.pos, src.mrgb)
        side = np.repeat(np.arange(len(pos)) % 2, rng.integers(1, 10, len(pos)))[:len(pos)]
        both = rng.random(len(pos)) < 0.05
        in_a, in_b = (side == 0) | both, (side == 1) | both
        oa, ob = rng.permutation(int(in_a.sum())), rng.permutation(int(in_b.sum()))
        add("alternating", (pos[in_a][oa], mrgb[in_a][oa]), (pos[in_b][ob], rng.integers(0, 256, (len(ob), 4)).astype(np.uint8)), runs=side)
    return tuple(out)


MORPH_BARS = (0, 1, 2, 8, 9, 10, 11, 12, 13)      # of LONG_KINDS: per axis the one-colour bar, a period of 2 047 to 2 049, the bit-7 bar


def connectivities(fam, k):
    """The connectivities at which a case goes through the morphology: its model's time goes with the cells times the rows, so a
    list of more than MORPH_WIDE distinct cells runs at 6 alone.  Of the full bars nine run, at 6 (the model takes 10 s for the
    four ops of one): on each axis the bar of one colour, one whose colour changes every 2 047, 2 048 or 2 049 cells (a wrong
    first source shows in a new cell's bytes) and the one whose colours differ in bit 7."""
    if fam == "long_runs":
        return (6,) if k in MORPH_BARS else ()
    return M.CONNECTIVITIES if len(distinct(case(fam, k).pos)) <= MORPH_WIDE else (6,)


# ---- the models' results, computed once ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def morphed(fam, k, op, c, steps=1, bare=False):
    """morph_model.morph of a case -> (pos, mrgb or None), shared and never written.  bare: positions only."""
    case_ = case(fam, k)
    return _frozen(*M.morph(case_.pos, None if bare else case_.mrgb, op, c, steps))


@functools.lru_cache(maxsize=None)
def morphed_piece(op, c, steps):
    """morph_model.morph of bar_piece()"""
    piece = bar_piece()
    return _frozen(*M.morph(piece.pos, piece.mrgb, op, c, steps))


@functools.lru_cache(maxsize=None)
def meshed(fam, k, mode, bare=False):
    """mesh_model.mesh of a case -> (verts, tris, tri_mrgb or None).  The bare result of a bar depends on its axis alone."""
    if fam == "long_runs" and bare and k >= 3:
        return meshed(fam, LONG_KINDS[k][1], mode, True)
    case_ = case(fam, k)
    return _frozen(*MM.mesh(case_.pos, None if bare else case_.mrgb, mode))


@functools.lru_cache(maxsize=None)
def combined(k, op, swapped=False, bare=False):
    """setops_model.combine of a pair (swapped: B with A) -> (pos, mrgb or None)"""
    pair = pairs()[k]
    a, b = (pair.b, pair.a) if swapped else (pair.a, pair.b)
    return _frozen(*S.combine(a[0], None if bare else a[1], b[0], None if bare else b[1], op))


# ---- classification, in numpy (no expected byte comes from here) ----------------------------------------------------------------------------
def u_of(pos):
    return np.asarray(pos, np.int64).reshape(-1, 3) + 32768


def trailing_ones(u):
    """the number of one bits at the low end of each u of 0 .. 65535 (16 for 65535)"""
    u = np.asarray(u, np.int64)
    return np.log2(((u ^ (u + 1)) + 1) >> 1).round().astype(np.int64)


def trailing_zeros(u):
    """the number of zero bits at the low end of each u of 0 .. 65535 (16 for 0)"""
    return trailing_ones((np.asarray(u, np.int64) - 1) % 65536)


def linear_keys(cells):
    c = np.asarray(cells, np.int64).reshape(-1, 3) + 32768
    return c[:, 0] << 32 | c[:, 1] << 16 | c[:, 2]


def listed_neighbour(cells, offset):
    """-> bool per distinct cell: the cell at `offset` from it is in range and listed"""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    q = cells + np.asarray(offset)
    ok = ((q >= LO) & (q <= HI)).all(axis=1)
    return ok & np.isin(linear_keys(np.clip(q, LO, HI)), linear_keys(cells))
