"""The rule of include/vxrt_transform.h in Python integers (no GPU needed).

The source is a dict from position to bytes filled in input order, so the last entry of a position wins; the box is walked cell by
cell; rule 2 is `>> 17` on Python ints, which neither wrap nor round towards zero; the range test is made on those ints; the result is
sorted by the path key at depth 15."""
import numpy as np

ONE = 65536
M_LIMIT, T_LIMIT = 1 << 24, 1 << 40
LO, HI = -32768, 32767


def path_key(p, depth=15):
    """device_build.h: path_key_of of u = p + 2^depth: bit k of u at bits 3k + 2 (x), 3k + 1 (y), 3k (z)."""
    half = 1 << depth
    ux, uy, uz = (int(v) + half for v in p)
    assert all(0 <= u < 2 * half for u in (ux, uy, uz))
    key = 0
    for k in range(depth + 1):
        key |= (((ux >> k) & 1) << 2 | ((uy >> k) & 1) << 1 | ((uz >> k) & 1)) << (3 * k)
    return key


def source_of(pos, mrgb=None):
    """Rule 1 -> {(x, y, z): (m & 0x7f, r, g, b)}, or {(x, y, z): None} without mrgb."""
    src = {}
    plist = np.asarray(pos).reshape(-1, 3).tolist()
    blist = [None] * len(plist) if mrgb is None else np.asarray(mrgb).reshape(-1, 4).tolist()
    for p, b in zip(plist, blist):
        src[tuple(p)] = None if b is None else (b[0] & 0x7F, b[1], b[2], b[3])
    return src


def pull_cell(m, t, d):
    """Rule 2 -> the source cell s of destination cell d, in Python ints."""
    c = [2 * int(v) + 1 for v in d]
    return tuple((int(m[i][0]) * c[0] + int(m[i][1]) * c[1] + int(m[i][2]) * c[2] + 2 * int(t[i])) >> 17 for i in range(3))


def in_range(s):
    return all(LO <= v <= HI for v in s)


def check_map(m, t):
    assert all(abs(int(v)) <= M_LIMIT for row in m for v in row) and all(abs(int(v)) <= T_LIMIT for v in t)


def transform(pos, mrgb, m, t, box_min, box_max, src=None):
    """Rules 1 to 4 -> (pos int16 [k,3], mrgb uint8 [k,4] or None).  src: source_of(pos, mrgb), where the caller has it."""
    check_map(m, t)
    src = source_of(pos, mrgb) if src is None else src
    out = []
    if src and all(int(box_min[ax]) < int(box_max[ax]) for ax in range(3)):
        for x in range(int(box_min[0]), int(box_max[0])):
            for y in range(int(box_min[1]), int(box_max[1])):
                for z in range(int(box_min[2]), int(box_max[2])):
                    s = pull_cell(m, t, (x, y, z))
                    if in_range(s) and s in src:
                        out.append(((x, y, z), src[s]))
    out.sort(key=lambda e: path_key(e[0]))
    out_pos = np.array([e[0] for e in out], np.int16).reshape(-1, 3)
    out_mrgb = None if mrgb is None else np.array([e[1] for e in out], np.uint8).reshape(-1, 4)
    return out_pos, out_mrgb


def transform_np(pos, mrgb, m, t, box_min, box_max):
    """transform() with the box walked by numpy in int64, which holds every |P| < 2^43 exactly and shifts arithmetically: what the
    GPU cases with large boxes compare with.  tests/test_transform_cpu.py holds it equal to transform()."""
    check_map(m, t)
    empty = (np.zeros((0, 3), np.int16), None if mrgb is None else np.zeros((0, 4), np.uint8))
    src = source_of(pos, mrgb)
    if not src or not all(int(box_min[ax]) < int(box_max[ax]) for ax in range(3)):
        return empty
    d = np.stack(np.meshgrid(*[np.arange(int(box_min[ax]), int(box_max[ax]), dtype=np.int64) for ax in range(3)], indexing="ij"), -1).reshape(-1, 3)
    c = 2 * d + 1
    mm, tt = np.array(m, np.int64), np.array(t, np.int64)
    s = (c @ mm.T + 2 * tt) >> 17
    ok = ((s >= LO) & (s <= HI)).all(axis=1)
    keys_of = lambda a: (a[:, 0] + 32768) << 32 | (a[:, 1] + 32768) << 16 | (a[:, 2] + 32768)     # noqa: E731
    spos = np.array(list(src), np.int64).reshape(-1, 3)
    skeys = keys_of(spos)
    order = np.argsort(skeys)
    skeys, spos = skeys[order], spos[order]
    at = np.searchsorted(skeys, keys_of(np.where(ok[:, None], s, 0)))
    at = np.minimum(at, len(skeys) - 1)
    hit = ok & (skeys[at] == keys_of(np.where(ok[:, None], s, 0)))
    d, at = d[hit], at[hit]
    by_path = sorted(range(len(d)), key=lambda i: path_key(d[i]))
    out_pos = d[by_path].astype(np.int16).reshape(-1, 3)
    if mrgb is None:
        return out_pos, None
    out_mrgb = np.array([src[tuple(p)] for p in spos[at][by_path].tolist()], np.uint8).reshape(-1, 4)
    return out_pos, out_mrgb


def identity():
    return [[ONE, 0, 0], [0, ONE, 0], [0, 0, ONE]], [0, 0, 0]


def scale(q16):
    return [[q16, 0, 0], [0, q16, 0], [0, 0, q16]], [0, 0, 0]


def translation(offset):
    """The pull of pos -> pos + offset (integers): s = d - offset."""
    return identity()[0], [-ONE * int(v) for v in offset]


def axis_rotations():
    """The 24 rotation matrices with entries in {0, 1, -1} and determinant 1, as lists of ints."""
    import itertools
    out = []
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            r = [[signs[i] if perm[i] == j else 0 for j in range(3)] for i in range(3)]
            if round(float(np.linalg.det(np.array(r, np.float64)))) == 1:
                out.append(r)
    assert len(out) == 24
    return out


def rotation_pull(r, twice_pivot=(0, 0, 0)):
    """The exact pull of x -> R (x - p) + p for an axis rotation R and a pivot p = twice_pivot / 2 (all integers or all half-integers):
    m = 65536 R^T, t = 65536 (p - R^T p), in integers."""
    rt = [[r[j][i] for j in range(3)] for i in range(3)]
    m = [[ONE * rt[i][j] for j in range(3)] for i in range(3)]
    t = [(ONE // 2) * (twice_pivot[i] - sum(rt[i][j] * twice_pivot[j] for j in range(3))) for i in range(3)]
    return m, t


# ---- the lists the tests share ---------------------------------------------------------------------------------------------------
def shell(half=8):
    """The shell one cell wide around [-half, half)^3, coloured by position -> (pos int16 [n,3], mrgb uint8 [n,4])."""
    g = np.arange(-half - 1, half + 1)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    cells = cells[((cells == -half - 1) | (cells == half)).any(axis=1)]
    mrgb = np.stack([(cells[:, 0] * 7 + 3) & 0xFF, (cells[:, 0] + 100) & 0xFF, (cells[:, 1] + 100) & 0xFF, (cells[:, 2] + 100) & 0xFF], -1)
    return cells.astype(np.int16), mrgb.astype(np.uint8)


def random_cells(seed=1, density=0.25):
    """tests/test_gpu_components.py's random_list: cells of [0, 40)^3 at a density, 5 % of them listed twice, shuffled, with random
    bytes (so the two entries of a repeated position differ) -> (pos int16 [n,3], mrgb uint8 [n,4])."""
    rng = np.random.default_rng(seed)
    cells = np.argwhere(rng.random((40, 40, 40)) < density)
    cells = np.concatenate([cells, cells[rng.integers(0, len(cells), len(cells) // 20)]])
    cells = cells[rng.permutation(len(cells))]
    return cells.astype(np.int16), rng.integers(0, 256, (len(cells), 4)).astype(np.uint8)


# Three general rotations (fixed; orthonormal to double precision): about (1, 2, 3) by 0.7 rad, about (-2, 1, 0.5) by 2.1 rad, about
# (0.3, -1, 0.2) by -1.3 rad.
def _about(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


GENERAL_ROTATIONS = (_about((1, 2, 3), 0.7), _about((-2, 1, 0.5), 2.1), _about((0.3, -1, 0.2), -1.3))
