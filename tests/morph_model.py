"""The rule of include/vxrt_morph.h in Python (no GPU needed).

The set is a dict from position to bytes filled in input order, so the last entry of a position wins (transform_model.source_of);
neighbours are looked up row by row from this file's own copy of the 26-row table; the steps are a loop, each on the result of the
one before; the result is sorted by the path key at depth 15 (transform_model.path_key)."""
import numpy as np

from transform_model import HI, LO, path_key, source_of

DILATE, ERODE, SURFACE, MARGIN = range(4)
OPS = (DILATE, ERODE, SURFACE, MARGIN)
NAMES = ("DILATE", "ERODE", "SURFACE", "MARGIN")
CONNECTIVITIES = (6, 18, 26)


def _table():
    """Rule 2: by the number of nonzero axes, then by 9 (dx + 1) + 3 (dy + 1) + (dz + 1)."""
    rows = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    rows.sort(key=lambda o: (sum(1 for d in o if d), 9 * (o[0] + 1) + 3 * (o[1] + 1) + (o[2] + 1)))
    return tuple(rows)


OFFSETS = _table()
assert len(OFFSETS) == 26 and OFFSETS[:6] == ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0))


def in_range(p):
    return all(LO <= v <= HI for v in p)


def neighbours(p, c):
    """The cells at rows 0 .. c - 1 from p, row by row; None where the cell lies outside the int16 range (it does not exist)."""
    out = []
    for o in OFFSETS[:c]:
        q = (p[0] + o[0], p[1] + o[1], p[2] + o[2])
        out.append(q if in_range(q) else None)
    return out


def dilate_once(s, c):
    """Rule 3 -> a new dict: s and every cell of the range with a neighbour in s, which takes the bytes of its first source."""
    cells = set()
    for p in s:
        cells.update(q for q in neighbours(p, c) if q is not None and q not in s)
    out = dict(s)
    for x in cells:
        out[x] = next(s[q] for q in neighbours(x, c) if q is not None and q in s)
    return out


def erode_once(s, c):
    return {p: b for p, b in s.items() if all(q is not None and q in s for q in neighbours(p, c))}


def morph_dict(s, op, c, steps):
    """Rules 2 to 4 on a dict position -> bytes (or None) -> the result as a dict, unordered."""
    assert op in OPS and c in CONNECTIVITIES and 1 <= steps <= 64
    cur = s
    for _ in range(steps):
        if not cur:
            break
        cur = dilate_once(cur, c) if op in (DILATE, MARGIN) else erode_once(cur, c)
    if op == SURFACE:
        return {p: b for p, b in s.items() if p not in cur}
    if op == MARGIN:
        return {p: b for p, b in cur.items() if p not in s}
    return cur


def morph(pos, mrgb, op, c=6, steps=1):
    """Rules 1 to 6 -> (pos int16 [k,3], mrgb uint8 [k,4] or None)."""
    out = morph_dict(source_of(pos, mrgb), op, c, steps)
    keys = sorted(out, key=path_key)
    out_pos = np.array(keys, np.int16).reshape(-1, 3)
    out_mrgb = None if mrgb is None else np.array([out[k] for k in keys], np.uint8).reshape(-1, 4)
    return out_pos, out_mrgb


def leaf_word(b):
    """device_build.h: leaf_word_of."""
    return 0x80000000 | (int(b[0]) & 0x7F) << 24 | int(b[1]) << 16 | int(b[2]) << 8 | int(b[3])


def word_bytes(w):
    return ((w >> 24) & 0x7F, (w >> 16) & 0xFF, (w >> 8) & 0xFF, w & 0xFF)


def key_cell(key, depth=15):
    """The inverse of transform_model.path_key."""
    u = [0, 0, 0]
    for k in range(depth + 1):
        o = (key >> (3 * k)) & 7
        u[0] |= ((o >> 2) & 1) << k
        u[1] |= ((o >> 1) & 1) << k
        u[2] |= (o & 1) << k
    half = 1 << depth
    return (u[0] - half, u[1] - half, u[2] - half)


def sorted_keys_words(pos, mrgb):
    """What the front of the call hands the steps: the ascending unique path keys of a list and their leaf words."""
    src = source_of(pos, mrgb)
    order = sorted(src, key=path_key)
    return [path_key(p) for p in order], [0 if src[p] is None else leaf_word(src[p]) for p in order]


def morph_keys(keys, words, op, c, steps):
    """The op on ascending unique keys with leaf words -> [(key, word)] ascending: what the steps must hand the decode."""
    s = {key_cell(k): w for k, w in zip(keys, words)}
    out = morph_dict(s, op, c, steps)
    return sorted((path_key(p), w) for p, w in out.items())


# ---- the lists the tests share ---------------------------------------------------------------------------------------------------
def cube16():
    """The solid cube [-8, 8)^3, coloured by position -> (pos int16 [4096,3], mrgb uint8 [4096,4])."""
    g = np.arange(-8, 8)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    mrgb = np.stack([(cells[:, 2] * 5 + 1) & 0xFF, (cells[:, 0] + 100) & 0xFF, (cells[:, 1] + 100) & 0xFF, (cells[:, 2] + 100) & 0xFF], -1)
    return cells.astype(np.int16), mrgb.astype(np.uint8)
