"""The rule of include/vxrt_shape.h in Python integers (no GPU needed).

inside() is rules 1 to 3 on Python ints, which neither wrap nor narrow; shape() walks the box cell by cell with it and sorts by the
path key at depth 15; shape_np() walks the box with numpy in int64 / uint64, which hold every value of the rule exactly (|P| < 2^43,
squares below 2^62 once rule 2 has passed), for boxes of up to a few million cells; tests/test_shape_cpu.py holds the two equal.
helper_box() is the box the host helpers must give."""
import math

import numpy as np

from transform_model import M_LIMIT, ONE, T_LIMIT, identity, path_key  # noqa: F401

BOX, BALL, CYLINDER, CAPSULE = 0, 1, 2, 3
LIMIT = 1 << 29          # r and h
NEAR = 1 << 31           # rule 2


def pulled(m, t, d):
    """Rule 1 -> (P_0, P_1, P_2), in Python ints."""
    c = [2 * int(v) + 1 for v in d]
    return tuple(int(m[i][0]) * c[0] + int(m[i][1]) * c[1] + int(m[i][2]) * c[2] + 2 * int(t[i]) for i in range(3))


def holds(kind, r, h, p):
    """Rules 2 and 3 for the pulled centre p."""
    if any(abs(v) >= NEAR for v in p):
        return False
    rr, hh = 2 * int(r), [2 * int(v) for v in h]
    if kind == BOX:
        return all(-hh[i] <= p[i] < hh[i] for i in range(3))
    if kind == BALL:
        return p[0] * p[0] + p[1] * p[1] + p[2] * p[2] <= rr * rr
    if kind == CYLINDER:
        return p[0] * p[0] + p[1] * p[1] <= rr * rr and -hh[2] <= p[2] < hh[2]
    assert kind == CAPSULE
    q = min(max(p[2], -hh[2]), hh[2])
    return p[0] * p[0] + p[1] * p[1] + (p[2] - q) ** 2 <= rr * rr


def inside(kind, r, h, m, t, d):
    return holds(kind, r, h, pulled(m, t, d))


def check_args(kind, r, h, m, t):
    assert kind in (BOX, BALL, CYLINDER, CAPSULE) and 0 <= r <= LIMIT and all(0 <= v <= LIMIT for v in h)
    assert all(abs(int(v)) <= M_LIMIT for row in m for v in row) and all(abs(int(v)) <= T_LIMIT for v in t)
    assert (r == 0) if kind == BOX else (h[0] == 0 and h[1] == 0)
    assert kind != BALL or h[2] == 0


def result(cells, mrgb):
    cells = sorted(cells, key=path_key)
    pos = np.array(cells, np.int16).reshape(-1, 3)
    if mrgb is None:
        return pos, None
    return pos, np.tile(np.array([[mrgb[0] & 0x7F, mrgb[1], mrgb[2], mrgb[3]]], np.uint8), (len(pos), 1)).reshape(-1, 4)


def shape(kind, r, h, m, t, box_min, box_max, mrgb=None):
    """Rules 1 to 5 -> (pos int16 [k,3], mrgb uint8 [k,4] or None)."""
    check_args(kind, r, h, m, t)
    out = []
    for x in range(int(box_min[0]), int(box_max[0])):
        for y in range(int(box_min[1]), int(box_max[1])):
            for z in range(int(box_min[2]), int(box_max[2])):
                if inside(kind, r, h, m, t, (x, y, z)):
                    out.append((x, y, z))
    return result(out, mrgb)


def path_keys_np(d):
    """path_key of every row of d (int64 [n,3]) -> uint64 [n]."""
    u = (d + 32768).astype(np.uint64)
    key = np.zeros(len(d), np.uint64)
    for k in range(16):
        for ax in range(3):
            key |= ((u[:, ax] >> np.uint64(k)) & np.uint64(1)) << np.uint64(3 * k + 2 - ax)
    return key


def shape_np(kind, r, h, m, t, box_min, box_max, mrgb=None):
    """shape() with the box walked by numpy.  Centres that fail rule 2 are set to 0 before anything is squared."""
    check_args(kind, r, h, m, t)
    if not all(int(box_min[ax]) < int(box_max[ax]) for ax in range(3)):
        return result([], mrgb)
    d = np.stack(np.meshgrid(*[np.arange(int(box_min[ax]), int(box_max[ax]), dtype=np.int64) for ax in range(3)], indexing="ij"), -1).reshape(-1, 3)
    p = (2 * d + 1) @ np.array(m, np.int64).T + 2 * np.array(t, np.int64)
    near = (np.abs(p) < NEAR).all(axis=1)
    p = np.where(near[:, None], p, 0)
    rr, hh = np.uint64((2 * int(r)) ** 2), [2 * int(v) for v in h]
    sq = lambda v: (v * v).astype(np.uint64)      # noqa: E731
    if kind == BOX:
        ok = np.ones(len(d), bool)
        for i in range(3):
            ok &= (-hh[i] <= p[:, i]) & (p[:, i] < hh[i])
    elif kind == BALL:
        ok = sq(p[:, 0]) + sq(p[:, 1]) + sq(p[:, 2]) <= rr
    elif kind == CYLINDER:
        ok = (sq(p[:, 0]) + sq(p[:, 1]) <= rr) & (-hh[2] <= p[:, 2]) & (p[:, 2] < hh[2])
    else:
        ok = sq(p[:, 0]) + sq(p[:, 1]) + sq(p[:, 2] - np.clip(p[:, 2], -hh[2], hh[2])) <= rr
    d = d[ok & near]
    d = d[np.argsort(path_keys_np(d), kind="stable")]
    pos = d.astype(np.int16).reshape(-1, 3)
    if mrgb is None:
        return pos, None
    return pos, np.tile(np.array([[mrgb[0] & 0x7F, mrgb[1], mrgb[2], mrgb[3]]], np.uint8), (len(pos), 1)).reshape(-1, 4)


def centred(c):
    """The identity map about the integer centre c: m = 65536 I, t = -65536 c."""
    return identity()[0], [-ONE * int(v) for v in c]


def q16(v):
    return int(np.rint(65536.0 * float(v)))


def helper_box(centre, extent):
    """[floor(centre - extent) - 2, ceil(centre + extent) + 2) clipped to [-32768, 32768]: what every host helper returns as its box
    for a shape with that half width per axis about that centre."""
    lo = tuple(int(min(max(math.floor(c - e) - 2, -32768), 32768)) for c, e in zip(centre, extent))
    hi = tuple(int(min(max(math.ceil(c + e) + 2, -32768), 32768)) for c, e in zip(centre, extent))
    return lo, hi


def unpack(H, made):
    """A helper's (Shape, Affine, box_min, box_max) -> (kind, r, h, m, t, box_min, box_max) in Python ints."""
    s, a, lo, hi = made
    assert isinstance(s, H.Shape) and isinstance(a, H.Affine) and list(s.reserved) == [0, 0, 0] and a.reserved == 0
    return int(s.kind), int(s.r), [int(v) for v in s.h], [[int(v) for v in row] for row in a.m], [int(v) for v in a.t], tuple(lo), tuple(hi)
