"""The rule of include/vxrt_distance.h in Python (no GPU needed).

distance() is the rule read literally, in Python integers: the set is a dict from position to bytes filled in input order, so the
last entry of a position wins (transform_model.source_of); every cell walks the cube of offsets with d2 <= max_d2 in the order of
rule 5's key (d2, rank(dz), rank(dy), rank(dx)) and stops at the first that answers it; the result is sorted by the path key at
depth 15 (transform_model.path_key).  distance_np() is the same walk with numpy doing the inner loops over sorted position codes,
for the lists of the GPU tests; tests/test_distance_cpu.py holds the two equal."""
import numpy as np

from transform_model import HI, LO, path_key, source_of

DEPTH, FIELD, ERODE, DILATE = range(4)
MODES = (DEPTH, FIELD, ERODE, DILATE)
NAMES = ("DEPTH", "FIELD", "ERODE", "DILATE")
FAR = 0xFFFF
MAX_D2 = 256


def rank(d):
    """Rule 5."""
    return 0 if d == 0 else -2 * d - 1 if d < 0 else 2 * d


def radius(max_d2):
    """Rule 2: the largest R with R * R <= max_d2."""
    r = 0
    while (r + 1) * (r + 1) <= max_d2:
        r += 1
    return r


_OFFSETS = {}


def offsets(max_d2):
    """Every (dx, dy, dz) with d2 <= max_d2, (0, 0, 0) included, in the order of rule 5's key."""
    if max_d2 not in _OFFSETS:
        r = radius(max_d2)
        g = range(-r, r + 1)
        cube = [(dx, dy, dz) for dx in g for dy in g for dz in g if dx * dx + dy * dy + dz * dz <= max_d2]
        cube.sort(key=lambda o: (o[0] * o[0] + o[1] * o[1] + o[2] * o[2], rank(o[2]), rank(o[1]), rank(o[0])))
        _OFFSETS[max_d2] = tuple(cube)
    return _OFFSETS[max_d2]


def in_range(p):
    return all(LO <= v <= HI for v in p)


def depth_of(s, v, max_d2):
    """Rule 4: the least d2 from voxel v to an empty cell (a cell outside the range is one), or FAR."""
    for o in offsets(max_d2):
        e = (v[0] + o[0], v[1] + o[1], v[2] + o[2])
        if not in_range(e) or e not in s:
            return o[0] * o[0] + o[1] * o[1] + o[2] * o[2]
    return FAR


def source_of_cell(s, x, max_d2):
    """Rules 4 and 5: (d2, source) of cell x, or None where no voxel lies within max_d2."""
    for o in offsets(max_d2):
        q = (x[0] + o[0], x[1] + o[1], x[2] + o[2])
        if q in s:                      # a position outside the range is in no set
            return o[0] * o[0] + o[1] * o[1] + o[2] * o[2], q
    return None


def distance_dict(s, mode, max_d2):
    """Rules 2 to 6 on a dict position -> bytes (or None) -> {position: (bytes, d2)}, unordered."""
    assert mode in MODES and 1 <= max_d2 <= MAX_D2
    out = {}
    if mode in (DEPTH, ERODE):
        for v, b in s.items():
            d = depth_of(s, v, max_d2)
            if mode == DEPTH or d > max_d2:
                out[v] = (b, d)
        return out
    cells = set()
    for v in s:
        for o in offsets(max_d2):
            x = (v[0] - o[0], v[1] - o[1], v[2] - o[2])
            if in_range(x) and x not in s:
                cells.add(x)
    for x in cells:
        d, q = source_of_cell(s, x, max_d2)
        out[x] = (s[q], d)
    if mode == DILATE:
        for v, b in s.items():
            out[v] = (b, 0)
    return out


def _arrays(out, with_bytes):
    keys = sorted(out, key=path_key)
    pos = np.array(keys, np.int16).reshape(-1, 3)
    mrgb = np.array([out[k][0] for k in keys], np.uint8).reshape(-1, 4) if with_bytes else None
    return pos, mrgb, np.array([out[k][1] for k in keys], np.uint16)


def distance(pos, mrgb, mode, max_d2):
    """Rules 1 to 8 -> (pos int16 [k,3], mrgb uint8 [k,4] or None, d2 uint16 [k])."""
    return _arrays(distance_dict(source_of(pos, mrgb), mode, max_d2), mrgb is not None)


def close_ball(pos, mrgb, max_d2, fn=None):
    fn = fn or distance_np
    return fn(*fn(pos, mrgb, DILATE, max_d2)[:2], ERODE, max_d2)[:2]


def open_ball(pos, mrgb, max_d2, fn=None):
    fn = fn or distance_np
    return fn(*fn(pos, mrgb, ERODE, max_d2)[:2], DILATE, max_d2)[:2]


# ---- the same walk with numpy ---------------------------------------------------------------------------------------------------
def _spread(v):
    x = v.astype(np.uint64)
    for shift, mask in ((32, 0x1F00000000FFFF), (16, 0x1F0000FF0000FF), (8, 0x100F00F00F00F00F), (4, 0x10C30C30C30C30C3), (2, 0x1249249249249249)):
        x = (x | (x << np.uint64(shift))) & np.uint64(mask)
    return x


def path_keys_np(cells):
    """transform_model.path_key of every row of cells (int [k,3])."""
    u = np.asarray(cells, np.int64).reshape(-1, 3) + 32768
    return (_spread(u[:, 0]) << np.uint64(2)) | (_spread(u[:, 1]) << np.uint64(1)) | _spread(u[:, 2])


def _code(u):
    """One integer per position u = p + 32768 (int64 [..., 3], each of 0 .. 65535)."""
    return (u[..., 0] << 32) | (u[..., 1] << 16) | u[..., 2]


def _member(sorted_codes, codes):
    at = np.minimum(np.searchsorted(sorted_codes, codes), len(sorted_codes) - 1)
    return sorted_codes[at] == codes


def _inside(u):
    return ((u >= 0) & (u <= 65535)).all(axis=-1)


_DEPTHS = {}


def distance_np(pos, mrgb, mode, max_d2, budget=1 << 21):
    """distance() for larger lists."""
    assert mode in MODES and 1 <= max_d2 <= MAX_D2
    with_bytes = mrgb is not None
    src = source_of(pos, mrgb)
    empty = (np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8) if with_bytes else None, np.zeros(0, np.uint16))
    if not src:
        return empty
    cells = np.array(list(src), np.int64).reshape(-1, 3) + 32768
    order = np.argsort(_code(cells))
    cells = cells[order]
    codes = _code(cells)
    bytes_ = np.array([src[k] for k in src], np.uint8).reshape(-1, 4)[order] if with_bytes else None
    offs = np.array(offsets(max_d2), np.int64)
    d2s = (offs * offs).sum(axis=1)

    def present(u):          # u int64 [..., 3]: in the range and in S
        ok = _inside(u)
        return ok & _member(codes, _code(np.clip(u, 0, 65535)))

    if mode in (DEPTH, ERODE):
        depth = np.full(len(cells), FAR, np.int64)
        memo = (codes.tobytes(), max_d2)                  # DEPTH and ERODE of one set walk the same offsets
        left = np.arange(len(cells)) if memo not in _DEPTHS else np.zeros(0, np.int64)
        for d in np.unique(d2s):
            if d == 0 or not len(left):
                continue
            group = offs[d2s == d]
            rows = max(1, budget // len(group))
            hit = np.concatenate([(~present(cells[left[i:i + rows], None, :] + group[None])).any(axis=1) for i in range(0, len(left), rows)])
            depth[left[hit]] = d
            left = left[~hit]
        if memo in _DEPTHS:
            depth = _DEPTHS[memo]
        elif len(cells) >= 4096:
            _DEPTHS.clear()
            _DEPTHS[memo] = depth
        keep = np.ones(len(cells), bool) if mode == DEPTH else depth > max_d2
        out_cells, out_d2, out_bytes = cells[keep], depth[keep], (bytes_[keep] if with_bytes else None)
    else:
        # a cell's nearest voxel has the cell's side empty: only voxels with an empty face neighbour are sources
        faces = np.array([(-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)], np.int64)
        surface = np.flatnonzero((~present(cells[:, None, :] + faces[None])).any(axis=1))
        ring = offs[1:]                                   # without (0, 0, 0); the priority is the index
        best_packed, best_src = np.zeros(0, np.int64), np.zeros(0, np.int64)
        rows = max(1, budget // len(ring))
        for i in range(0, len(surface), rows):
            part = surface[i:i + rows]
            x = cells[part, None, :] - ring[None]        # (dx, dy, dz) = s - x
            ok = _inside(x)
            ok &= ~_member(codes, _code(np.clip(x, 0, 65535)))
            packed = (_code(x) << 15) | np.arange(len(ring), dtype=np.int64)[None]
            who = np.broadcast_to(part[:, None], ok.shape)
            best_packed = np.concatenate([best_packed, packed[ok]])
            best_src = np.concatenate([best_src, who[ok]])
            o = np.argsort(best_packed, kind="stable")
            best_packed, best_src = best_packed[o], best_src[o]
            first = np.ones(len(best_packed), bool)
            first[1:] = (best_packed[1:] >> 15) != (best_packed[:-1] >> 15)
            best_packed, best_src = best_packed[first], best_src[first]
        code = best_packed >> 15
        out_cells = np.stack([code >> 32, (code >> 16) & 0xFFFF, code & 0xFFFF], -1)
        out_d2 = d2s[1:][best_packed & 0x7FFF]
        out_bytes = bytes_[best_src] if with_bytes else None
        if mode == DILATE:
            out_cells = np.concatenate([cells, out_cells])
            out_d2 = np.concatenate([np.zeros(len(cells), np.int64), out_d2])
            out_bytes = np.concatenate([bytes_, out_bytes]) if with_bytes else None
    if not len(out_cells):
        return empty
    by_path = np.argsort(path_keys_np(out_cells - 32768))
    return ((out_cells[by_path] - 32768).astype(np.int16), out_bytes[by_path] if with_bytes else None, out_d2[by_path].astype(np.uint16))


# ---- the lists the tests share ---------------------------------------------------------------------------------------------------
def solid(side, origin=0):
    """The solid cube [origin, origin + side)^3, coloured by position -> (pos int16 [side^3,3], mrgb uint8 [side^3,4])."""
    g = np.arange(origin, origin + side)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    mrgb = np.stack([(cells[:, 2] * 5 + 1) & 0xFF, (cells[:, 0] + 100) & 0xFF, (cells[:, 1] + 100) & 0xFF, (cells[:, 2] + 100) & 0xFF], -1)
    return cells.astype(np.int16), mrgb.astype(np.uint8)
