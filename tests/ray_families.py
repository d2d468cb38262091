"""Rays the octree walk dislikes, by family, the scenes they are sent through, and the ray-by-ray comparison (no GPU needed).

World units: voxel p of vxrt_set_voxels is the cube [p / 2, p / 2 + 1/2)^3, so every node plane of every level is a multiple of 0.5
and the root cube of a depth-d scene is [-2^d / 2, 2^d / 2)^3.  tests/test_ray_families_cpu.py checks with the oracle alone that each
family is what it claims; tests/test_gpu_ray_walk.py sends them through every walk of the device."""
import numpy as np

f32 = np.float32
N_RAYS = 20000          # rays per family in both test files
SEED = 20240

FAMILIES = ("on_planes", "ulp_off_planes", "zero_components", "scaled_dirs", "tiny_component", "root_faces", "far_origins",
            "inside_solid", "nonfinite_origin", "nonfinite_dir")
SCENES = ("cube16", "cube32", "castle", "one_voxel", "empty", "deep15")


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
def _cube(half, seed):
    """A random half of [-half, half)^3 plus its eight corners: touches every face of its root, all eight root slots occupied."""
    rng = np.random.default_rng(seed)
    g = np.arange(-half, half)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    keep = rng.random(len(cells)) < 0.5
    keep |= np.all((cells == -half) | (cells == half - 1), axis=1)
    pos = cells[keep].astype(np.int16)
    mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    mrgb[:, 0] = np.where(rng.random(len(pos)) < 0.1, 0x40, 0)      # a tenth emits
    return pos, mrgb


def scene_voxels(name, scenes=None):
    """-> (pos int16[n,3], mrgb uint8[n,4]).  `scenes`: gpu_voxel_raytracer_amd.scenes (castle only)."""
    if name == "cube16":
        return _cube(8, 16)       # depth 3: node levels 0 .. 3
    if name == "cube32":
        return _cube(16, 32)      # depth 4: node levels 0 .. 4 (the wide records see an odd and an even level count)
    if name == "castle":          # positive octant: a root with one occupied slot
        pos, mrgb, _ = scenes.load_scene("castle")
        return np.ascontiguousarray(pos, np.int16), np.ascontiguousarray(mrgb, np.uint8)
    if name == "one_voxel":
        return np.array([[-1, -1, -1]], np.int16), np.array([[0, 1, 2, 3]], np.uint8)
    if name == "empty":
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    if name == "deep15":          # the deepest tree int16 coordinates allow
        return np.array([[32767, 3, -2], [0, 0, 0]], np.int16), np.array([[0, 10, 200, 30], [0x40, 255, 255, 255]], np.uint8)
    raise KeyError(name)


def world_box(pos):
    """The voxels' box in world units (an empty scene: its depth-0 root cube)."""
    if len(pos) == 0:
        return np.full(3, -0.5), np.full(3, 0.5)
    p = np.asarray(pos, np.float64)
    return p.min(0) * 0.5, (p.max(0) + 1.0) * 0.5


def root_half_of(octree):
    """Half the root cube's edge, from the header of the oracle's octree buffer (centre xyz, size, ...)."""
    return float(np.asarray(octree[:5], np.int32).view(f32)[3]) * 0.5


def leaf_words(pos, mrgb):
    """The voxel model {(x, y, z): leaf word as int32}: 0x80000000 | (material & 0x7f) << 24 | rgb; the last entry of a position wins."""
    m = np.asarray(mrgb, np.uint32)
    w = (np.uint32(0x80000000) | (m[:, 0] & 0x7F) << 24 | m[:, 1] << 16 | m[:, 2] << 8 | m[:, 3]).astype(np.uint32).view(np.int32)
    return {tuple(p): int(v) for p, v in zip(np.asarray(pos).tolist(), w.tolist())}


# ---- the families ------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(f32)


def _snap(x):
    return np.round(np.asarray(x, np.float64) * 2.0) / 2.0


def _plane_origins(rng, lo, hi, n, p_snap=0.6):
    ext = hi - lo
    o = rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, (n, 3))
    return np.where(rng.random((n, 3)) < p_snap, _snap(o), o).astype(f32)


def _signed_zero(rng, shape):
    return np.where(rng.random(shape) < 0.5, f32(0.0), f32(-0.0)).astype(f32)


def _poison(rng, a):
    """30 % of the coordinates, and at least one per ray, become NaN, +inf or -inf."""
    n = len(a)
    bad = rng.random((n, 3)) < 0.3
    none = ~bad.any(1)
    bad[np.flatnonzero(none), rng.integers(0, 3, int(none.sum()))] = True
    what = np.array([np.nan, np.inf, -np.inf], f32)[rng.integers(0, 3, (n, 3))]
    return np.where(bad, what, a).astype(f32)


def families(rng, lo, hi, root_half, n, voxels=None):
    """-> {name: (origins float32[n,3], dirs float32[n,3])}, deterministic for a seeded `rng`.  lo / hi: the scene's world box;
    root_half: half the root cube's edge; voxels: the scene's positions (int[k,3]) for `inside_solid`, which is left out without any."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    out = {}
    # origins exactly on voxel planes (and so on node planes of every level), unit directions
    out["on_planes"] = (_plane_origins(rng, lo, hi, n), _unit(rng, n))
    # every coordinate on a plane, then one ulp beside it
    o = _plane_origins(rng, lo, hi, n, p_snap=2.0)
    toward = np.where(rng.random((n, 3)) < 0.5, f32(np.inf), f32(-np.inf)).astype(f32)
    out["ulp_off_planes"] = (np.nextafter(o, toward).astype(f32), _unit(rng, n))
    # direction components that are exactly +0 or -0 (never all three); 30 % exact axis directions with signed zeros kept
    d = rng.normal(size=(n, 3)).astype(f32)
    zero = rng.random((n, 3)) < 0.45
    zero[zero.all(1), 0] = False
    d = np.where(zero, _signed_zero(rng, (n, 3)), d).astype(f32)
    axis = rng.random(n) < 0.3
    lead = np.argmax(np.abs(d), axis=1)
    ax = _signed_zero(rng, (n, 3))
    ax[np.arange(n), lead] = np.sign(d[np.arange(n), lead])
    d = np.where(axis[:, None], ax, d).astype(f32)
    out["zero_components"] = (_plane_origins(rng, lo, hi, n), d)
    # unnormalised directions of magnitude 1e-44 .. 1e37: subnormal components make 1/d infinite, large ones make it subnormal
    with np.errstate(under="ignore"):
        d = (_unit(rng, n).astype(np.float64) * 10.0 ** rng.uniform(-44.0, 37.0, (n, 1))).astype(f32)
    out["scaled_dirs"] = (_plane_origins(rng, lo, hi, n), d)
    # one component of magnitude 1e-45 .. 1e-30, the rest of a unit vector
    d = _unit(rng, n)
    with np.errstate(under="ignore"):
        tiny = (10.0 ** rng.uniform(-45.0, -30.0, n) * rng.choice([-1.0, 1.0], n)).astype(f32)
    d[np.arange(n), rng.integers(0, 3, n)] = tiny
    out["tiny_component"] = (_plane_origins(rng, lo, hi, n), d)
    # origins on the root cube's faces, edges, corners and centre planes
    r = float(root_half)
    o = np.array([-r, -r / 2, 0.0, r / 2, r], f32)[rng.integers(0, 5, (n, 3))]
    out["root_faces"] = (o, _unit(rng, n))
    # origins 1e1 .. 1e30 away, aimed at a point of the box
    u = _unit(rng, n)
    target = rng.uniform(lo, hi, (n, 3))
    o = (target - u.astype(np.float64) * 10.0 ** rng.uniform(1.0, 30.0, (n, 1))).astype(f32)
    out["far_origins"] = (o, u)
    # origins at centres, face centres and corners of occupied voxels
    if voxels is not None and len(voxels):
        v = np.asarray(voxels, np.float64)[rng.integers(0, len(voxels), n)]
        kind = rng.integers(0, 3, n)
        off = np.full((n, 3), 0.25)
        face = rng.choice([0.0, 0.5], n)
        k = rng.integers(0, 3, n)
        is_face = kind == 1
        off[np.flatnonzero(is_face), k[is_face]] = face[is_face]
        corner = rng.choice([0.0, 0.5], (n, 3))
        off = np.where((kind == 2)[:, None], corner, off)
        out["inside_solid"] = ((v * 0.5 + off).astype(f32), _unit(rng, n))
    out["nonfinite_origin"] = (_poison(rng, _plane_origins(rng, lo, hi, n)), _unit(rng, n))
    out["nonfinite_dir"] = (_plane_origins(rng, lo, hi, n), _poison(rng, _unit(rng, n)))
    return out


def scene_families(name, pos, root_half, n=N_RAYS):
    """The families of scene `name`, the same rays wherever they are asked for."""
    lo, hi = world_box(pos)
    return families(np.random.default_rng([SEED, SCENES.index(name)]), lo, hi, root_half, n, voxels=pos)


def is_regular(dirs):
    """ray_is_regular (csrc/trace_common.h) per ray: every component of fl(1 / d) is finite and non-zero.  Such rays take the walk
    with the plane times kept in registers, all others the walk that follows the shader's text."""
    with np.errstate(divide="ignore", over="ignore", under="ignore", invalid="ignore"):
        inv = np.abs(f32(1.0) / np.asarray(dirs, f32))
    return np.all((inv > 0) & (inv < np.inf), axis=1)


# ---- comparison --------------------------------------------------------------------------------------------------------------------
def _u32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def differing_rays(got, want):
    """got / want: (hit, time, leaf word, normal[n,3]) -> bool[n], true where anything differs: the hit flag, the time's bits (NaN
    equals NaN), the leaf word, the normal's bits (signs of zero included).  The time of a miss counts: it is what
    cast_bounded_ray leaves in `time`."""
    gh, gt, gn, gm = got
    wh, wt, wn, wm = want
    gt, wt = np.asarray(gt, f32), np.asarray(wt, f32)
    gm, wm = np.asarray(gm, f32).reshape(-1, 3), np.asarray(wm, f32).reshape(-1, 3)
    t_same = (_u32(gt) == _u32(wt)) | (np.isnan(gt) & np.isnan(wt))
    m_same = ((_u32(gm) == _u32(wm)) | (np.isnan(gm) & np.isnan(wm))).all(1)
    leaf_same = np.asarray(gn).astype(np.int64) == np.asarray(wn).astype(np.int64)
    return (np.asarray(gh, bool) != np.asarray(wh, bool)) | ~t_same | ~leaf_same | ~m_same


def zero_time_sign_rays(got, want, origins):
    """-> bool[n]: the rays whose device result differs from the oracle's in NOTHING but the sign bit of a zero time — device -0,
    oracle +0 — and whose origin has a coordinate exactly on a multiple of the finest cell (0.5): the pinned difference (DESIGN.md
    section 2: v_min3 orders -0 below +0 where the shader's min keeps its first operand)."""
    gh, gt, gn, gm = got
    wh, wt, wn, wm = want
    flipped = (_u32(gt) == 0x80000000) & (_u32(wt) == 0)
    as_want = (np.asarray(gh, bool), np.where(flipped, f32(0.0), np.asarray(gt, f32)).astype(f32), gn, gm)
    o = np.asarray(origins, np.float64)
    on_plane = (np.isfinite(o) & (o * 2.0 == np.round(o * 2.0))).any(1)
    return flipped & ~differing_rays(as_want, want) & on_plane


def _hex3(v):
    return "(" + ", ".join(f"0x{int(b):08x}" for b in _u32(v).ravel()) + ")"


def assert_rays_equal(got, want, what, origins=None, dirs=None, show=8, zero_time_sign=False):
    """Every ray equal (differing_rays).  zero_time_sign: the rays of zero_time_sign_rays are let through, and counted -> their number."""
    bad = differing_rays(got, want)
    pinned = 0
    if zero_time_sign and bad.any():
        let = zero_time_sign_rays(got, want, origins)
        pinned = int(let.sum())
        bad &= ~let
    if not bad.any():
        return pinned
    lines = [f"{what}: {int(bad.sum())} of {len(bad)} rays differ"]
    for i in np.flatnonzero(bad)[:show]:
        ray = "" if origins is None else f" o {_hex3(origins[i])} {np.asarray(origins[i]).tolist()} d {_hex3(dirs[i])} {np.asarray(dirs[i]).tolist()}"
        side = [f"hit {bool(r[0][i])} t {_hex3(np.asarray(r[1])[i])} leaf 0x{int(r[2][i]) & 0xffffffff:08x} n {_hex3(np.asarray(r[3])[i])}" for r in (got, want)]
        lines.append(f"  ray {i}:{ray}\n     got  {side[0]}\n     want {side[1]}")
    raise AssertionError("\n".join(lines))


# ---- what the oracle gives at N_RAYS rays per family with SEED (tests/test_ray_families_cpu.py asserts it) -------------------------
# (scene, family) -> hit floor: half the hits measured at this size, rounded down to two digits.  Pairs with fewer than 100 hits are
# left out: everything on the empty scene, most of deep15 (two voxels in a cube 16 384 wide), and the two non-finite families on
# the scenes whose root has nothing on its low faces (see ALL_MISS).
HIT_FLOOR = {
    ("cube16", "on_planes"): 7000, ("cube16", "ulp_off_planes"): 6800, ("cube16", "zero_components"): 6500, ("cube16", "scaled_dirs"): 5800,
    ("cube16", "tiny_component"): 6600, ("cube16", "root_faces"): 7100, ("cube16", "far_origins"): 2300, ("cube16", "inside_solid"): 9800,
    ("cube16", "nonfinite_origin"): 1400, ("cube16", "nonfinite_dir"): 1400,
    ("cube32", "on_planes"): 7200, ("cube32", "ulp_off_planes"): 7100, ("cube32", "zero_components"): 6500, ("cube32", "scaled_dirs"): 5800,
    ("cube32", "tiny_component"): 6800, ("cube32", "root_faces"): 7200, ("cube32", "far_origins"): 2400, ("cube32", "inside_solid"): 9900,
    ("cube32", "nonfinite_origin"): 1400, ("cube32", "nonfinite_dir"): 1400,
    ("castle", "on_planes"): 4900, ("castle", "ulp_off_planes"): 5000, ("castle", "zero_components"): 4900, ("castle", "scaled_dirs"): 3700,
    ("castle", "tiny_component"): 4500, ("castle", "root_faces"): 470, ("castle", "far_origins"): 2200, ("castle", "inside_solid"): 9500,
    ("one_voxel", "on_planes"): 5100, ("one_voxel", "ulp_off_planes"): 3000, ("one_voxel", "zero_components"): 3600,
    ("one_voxel", "scaled_dirs"): 4900, ("one_voxel", "tiny_component"): 4700, ("one_voxel", "root_faces"): 480,
    ("one_voxel", "far_origins"): 2000, ("one_voxel", "inside_solid"): 7200,
    ("deep15", "zero_components"): 170, ("deep15", "inside_solid"): 7200,
}
# A NaN coordinate is dropped by the shader's compare-and-select max / min unless it is the FIRST operand (x), where it makes the root
# test fail; an infinite one always makes it fail.  A ray with a NaN in y or z (origin or direction) therefore enters the root, and
# current_octant's strict > sends it to the LOW side of that axis at every level: it can only hit voxels on the root's low face.
# cube16 and cube32 have such voxels (both families hit there, HIT_FLOOR above); in these scenes nothing is reachable that way
# and every ray of the two families misses, exactly:
ALL_MISS = tuple((s, f) for s in ("castle", "one_voxel", "empty", "deep15") for f in ("nonfinite_origin", "nonfinite_dir"))
# rays a family must put into each walk: family -> (least regular rays, least other rays); 0: none at all, exactly
WALK_SPLIT = {
    "on_planes": (N_RAYS, 0), "ulp_off_planes": (N_RAYS, 0), "root_faces": (N_RAYS, 0), "far_origins": (N_RAYS, 0),
    "inside_solid": (N_RAYS, 0), "nonfinite_origin": (N_RAYS, 0), "nonfinite_dir": (0, N_RAYS),
    "zero_components": (1000, 10000),   # mostly the shader-text walk; the rays that drew no zero stay regular
    "scaled_dirs": (10000, 1000),       # |d| below ~3e-39: 1/d overflows
    "tiny_component": (5000, 5000),     # the tiny component's reciprocal is finite above ~3e-39 only
}
