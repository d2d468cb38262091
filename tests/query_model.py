"""The rules of include/vxrt_query.h in Python (no GPU needed).

Lookup: a voxel model {(x, y, z): leaf word} (ray_families.leaf_words) asked at pos + offset in Python integers, so nothing wraps; a
position outside the root cube [-2^d, 2^d)^3 answers 0.  Rays: the oracle's cast_rays(octree, o, d, max_distance), which takes one
bound per call, so the rays are grouped by the bits of their max_time (NaN is a bound like any other)."""
import numpy as np

f32 = np.float32
UNBOUNDED = float(1 << 30)           # the shader's ALMOST_INFINITY
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def lookup(model, depth, pos, offset=None):
    """-> (leaf int32[n], n_present).  model: {(x, y, z): int32 leaf word}; depth: the scene's octree depth."""
    off = (0, 0, 0) if offset is None else tuple(int(v) for v in offset)
    assert len(off) == 3 and all(INT32_MIN <= v <= INT32_MAX for v in off)
    half = 1 << int(depth)
    out = np.zeros(len(pos), np.int32)
    for i, p in enumerate(np.asarray(pos).reshape(-1, 3).tolist()):
        q = (p[0] + off[0], p[1] + off[1], p[2] + off[2])
        if all(-half <= v < half for v in q):
            out[i] = model.get(q, 0)
    return out, int(np.count_nonzero(out))


def cast(O, octree, origins, dirs, max_time=None):
    """-> (hit bool[n], time f32[n], leaf int32[n], normal f32[n,3]) of cast_bounded_ray with max_distance = max_time[i] (None: 2^30)."""
    o = np.ascontiguousarray(origins, f32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, f32).reshape(-1, 3)
    n = len(o)
    if max_time is None:
        return O.cast_rays(octree, o, d)[:4]
    t = np.ascontiguousarray(np.broadcast_to(np.asarray(max_time, f32), (n,)), f32)
    hit, time, leaf, normal = np.zeros(n, bool), np.zeros(n, f32), np.zeros(n, np.int32), np.zeros((n, 3), f32)
    bits = t.view(np.uint32)
    for b in np.unique(bits):
        at = np.flatnonzero(bits == b)
        bound = float(np.array([b], np.uint32).view(f32)[0])
        h, tm, lf, nm = O.cast_rays(octree, o[at], d[at], bound)[:4]
        hit[at], time[at], leaf[at], normal[at] = h, tm, lf, nm
    return hit, time, leaf, normal


BOUNDS = ("zero", "quarter", "one", "half_root", "unbounded", "negative", "nan")


def dealt_bounds(n, root_half):
    """The seven bounds of the GPU test dealt round-robin over n rays -> float32[n]: 0, 0.25, 1, half the root edge, 2^30, -1, NaN."""
    values = np.array([0.0, 0.25, 1.0, float(root_half), UNBOUNDED, -1.0, np.nan], f32)
    return values[np.arange(n) % len(values)].copy()
