"""Synthetic inputs for the temporal stage and a float64 model of it (no tests here).

The scene: a few axis-aligned boxes (a back wall, a floor, two blocks) cast in float64 from an old and a new camera, rounded to
binary32, so that most pixels of the new frame reproject onto matching history.  On top of that, chosen sparse subsets of both
frames are salted with what the tracer never produces: sky and zero / NaN / inf depths, non-finite colours, odd normals in the
current frame; non-finite colours, blending factors off the 1, 1/2, 1/4, ... ladder and depths beyond the cutoff in the history.

temporal_f64 restates shaders/temporal.comp:48-125 in float64 from the shader's text:
  * the inverse of the old screen-to-world matrix (temporal.comp:75-82) is numpy.linalg.inv of the 4x4 matrix;
  * texture() (temporal.comp:94, 113) is Vulkan's linear filter with clamp-to-edge: texel coordinate u * w - 0.5, weights rounded
    to 8 fractional bits, and a texel whose weight is 0 is not read (the project's rule, oracle U4).
Where GLSL leaves the result undefined (NaN through clamp, mix with an infinite operand), the pixel is marked not comparable.
"""
import numpy as np

SKY_NORMAL = np.float32(2.0 ** 30)     # what the trace stage writes for a miss: normal 2^30, depth -1
LADDER = np.array([1.0, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.02], np.float32)
OFF_LADDER = np.array([0.0, 0.3, 1.0, 1.5, -0.25, np.nan, np.inf], np.float32)

# (lo, hi) of each box; the camera looks along +z from near the origin
BOXES = (
    ((-60.0, -60.0, 14.0), (60.0, 3.1, 15.0)),        # back wall (top edge below the top of the view: sky above it)
    ((-60.0, -3.3, -60.0), (60.0, -2.3, 14.5)),       # floor, reaching far behind the cameras
    ((-2.7, -2.3, 5.1), (-0.6, 0.9, 6.9)),            # a block on the floor
    ((0.9, -2.3, 8.3), (3.3, 1.7, 9.7)),              # a taller block further back
)
WALL_Z = 14.0

# motions: (old camera, new camera), each (position, direction, fov); see motion()
MOTIONS = ("rest", "drift", "pixel_pan", "rotation", "fov", "out_of_view", "behind")
FOV = float(np.float32(70.0) * (np.float32(np.pi) / np.float32(180.0)))


def cam16(O, pos, dirn, fov, w, h):
    """origin, right, up, forward_ray as 4 vec4 (the first 64 bytes of the uniforms), with the product's binary32 basis."""
    u = O.Uniforms.default()
    u.set_camera(np.asarray(pos, np.float32), O.camera_axis_scaled(np.asarray(pos, np.float32), np.asarray(dirn, np.float32), fov, w, h))
    return u.camera16()


def _rot(d, yaw, pitch):
    d = np.asarray(d, np.float64)
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    d = np.array([cy * d[0] + sy * d[2], d[1], -sy * d[0] + cy * d[2]])
    return np.array([d[0], cp * d[1] + sp * d[2], -sp * d[1] + cp * d[2]])


def motion(O, name, w, h):
    """-> (old camera, new camera) as (position, direction, fov) with float32 position and direction."""
    f32 = np.float32
    p0, d0 = np.array([0.13, 0.37, -0.45], f32), np.array([0.0, 0.0, 1.0], f32)
    old = (p0, d0, FOV)
    if name == "rest":
        new = old
    elif name == "drift":           # well under a pixel everywhere
        new = (p0 + np.array([0.0021, -0.0013, 0.0017], f32), d0, FOV)
    elif name == "pixel_pan":
        # the back wall is square to the view: moving the camera by whole pixels of the wall's plane shifts the wall by whole pixels,
        # so its reprojections land on texel centres (weights exactly 0 or 1)
        c = cam16(O, p0, d0, FOV, w, h)
        span = (WALL_Z - float(p0[2])) / float(c[14])
        new = (p0 + np.array([3 * c[4] * span, 2 * c[9] * span, 0.0]).astype(f32), d0, FOV)
    elif name == "rotation":
        new = (p0, _rot(d0, 0.031, -0.017).astype(f32), FOV)
    elif name == "fov":
        new = (p0, d0, float(np.float32(62.0) * (np.float32(np.pi) / np.float32(180.0))))
    elif name == "out_of_view":
        new = (p0 + np.array([0.4, 0.0, 0.2], f32), _rot(d0, 0.75, 0.05).astype(f32), FOV)
    elif name == "behind":          # backed off and turned down: the near floor lies behind the old camera
        new = (p0 + np.array([0.3, 0.6, -4.5], f32), _rot(d0, -0.05, 0.30).astype(f32), FOV)
    else:
        raise ValueError(name)
    return old, new


def pixel_dirs(c16, w, h):
    """float64 unit ray directions of every pixel: normalize(x * right - y * up + forward_ray)  (temporal.comp:62-67)."""
    c = np.asarray(c16, np.float64)
    r, u, f = c[4:7], c[8:11], c[12:15]
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = x[..., None] * r - y[..., None] * u + f
    return d / np.sqrt((d * d).sum(-1, keepdims=True))


def cast(c16, w, h):
    """normal/depth of the scene seen by a camera, cast in float64 and rounded to binary32 (misses as the trace stage writes them)."""
    o = np.asarray(c16, np.float64)[0:3]
    d = pixel_dirs(c16, w, h)
    best = np.full((h, w), np.inf)
    normal = np.zeros((h, w, 3))
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        for lo, hi in BOXES:
            t0, t1 = (np.asarray(lo) - o) * inv, (np.asarray(hi) - o) * inv
            tmin, tmax = np.minimum(t0, t1), np.maximum(t0, t1)
            enter, leave, axis = tmin.max(-1), tmax.min(-1), tmin.argmax(-1)
            hit = (enter <= leave) & (enter > 0) & (enter < best)
            best = np.where(hit, enter, best)
            n = np.zeros((h, w, 3))
            np.put_along_axis(n, axis[..., None], -np.sign(np.take_along_axis(d, axis[..., None], -1)), -1)
            normal = np.where(hit[..., None], n, normal)
    nd = np.zeros((h, w, 4), np.float32)
    sky = ~np.isfinite(best)
    nd[..., :3] = normal.astype(np.float32)
    nd[..., 3] = best.astype(np.float32)
    nd[sky, :3] = SKY_NORMAL
    nd[sky, 3] = -1.0
    return nd


def synthetic_frames(O, w, h, motion_name, seed, exotic=True):
    """-> dict(color, nd, alb: the current frame; old_color, old_nd: the history; cam, old_cam: cam16 of each; old/new: the cameras)."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    old, new = motion(O, motion_name, w, h)
    oc, nc = cam16(O, *old, w, h), cam16(O, *new, w, h)
    old_nd, nd = cast(oc, w, h), cast(nc, w, h)
    color = (rng.random((h, w, 4)) * 3.0).astype(f32)
    old_color = (rng.random((h, w, 4)) * 3.0).astype(f32)
    old_color[..., 3] = LADDER[rng.integers(0, len(LADDER), (h, w))]
    alb = rng.random((h, w, 4)).astype(f32)
    alb[..., 3] = (np.uint32(0x80000000) | rng.integers(0, 1 << 30, (h, w)).astype(np.uint32)).view(f32)
    if exotic:
        def pick(p):
            return rng.random((h, w)) < p
        # current frame
        s = pick(0.02)
        nd[s, :3], nd[s, 3] = SKY_NORMAL, -1.0
        for v in (0.0, -0.0, np.nan, np.inf):
            nd[pick(0.003), 3] = v
        for k, v in ((0, np.inf), (1, -np.inf), (2, np.nan)):
            color[pick(0.003), k] = v
        odd = pick(0.01)
        nd[odd, :3] = nd[odd, :3] * f32(1.7) + f32(0.2)                    # not unit length
        nd[pick(0.004), 1] = f32(-0.0)
        nd[pick(0.003), 2] = np.nan
        # history: non-finite colours in sparse texels (their neighbours reproject onto them), blending off the ladder,
        # depths pushed beyond any cutoff the GUI offers
        for k, v in ((0, np.nan), (1, np.inf), (2, -np.inf)):
            old_color[pick(0.002), k] = v
        for v in OFF_LADDER:
            old_color[pick(0.004), 3] = v
        far = pick(0.02) & (old_nd[..., 3] > 0)
        old_nd[far, 3] = old_nd[far, 3] * f32(1.5)
    return dict(color=color, nd=nd, alb=alb, old_color=old_color, old_nd=old_nd, cam=nc, old_cam=oc, old=old, new=new)


def _sample(img, u, v, pick):
    """texture() of img (float64[h, w, c]) at (u, v) for the pixels in `pick`: linear filter, clamp-to-edge, 8-bit weights, and a
    texel of weight 0 not read.  -> (value, fx, fy, ax, ay)."""
    h, w = img.shape[:2]
    fx, fy = np.where(pick, u * w - 0.5, 0.0), np.where(pick, v * h - 0.5, 0.0)
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = np.floor((fx - x0) * 256.0 + 0.5) / 256.0, np.floor((fy - y0) * 256.0 + 0.5) / 256.0
    xa, xb = np.clip(x0, 0, w - 1).astype(np.int64), np.clip(x0 + 1, 0, w - 1).astype(np.int64)
    ya, yb = np.clip(y0, 0, h - 1).astype(np.int64), np.clip(y0 + 1, 0, h - 1).astype(np.int64)
    t00, t10, t01, t11 = img[ya, xa], img[ya, xb], img[yb, xa], img[yb, xb]
    axe, aye = ax[..., None], ay[..., None]
    with np.errstate(invalid="ignore"):
        top = np.where(axe == 0, t00, np.where(axe == 1, t10, t00 * (1 - axe) + t10 * axe))
        bot = np.where(axe == 0, t01, np.where(axe == 1, t11, t01 * (1 - axe) + t11 * axe))
        out = np.where(aye == 0, top, np.where(aye == 1, bot, top * (1 - aye) + bot * aye))
    return out, fx, fy, ax, ay


def _near_int(x, m):
    with np.errstate(invalid="ignore"):
        return np.abs(x - np.round(x)) < m


def temporal_f64(color, nd, old_color, old_nd, c16, old_c16, tu, safety=1.0, margin_rel=2e-4):
    """float64 temporal.comp:48-125 with a history.  tu: sample_blending, maximum_blending, blending_distance_cutoff (any object
    with those attributes).  A pixel is fragile when a binary32 evaluation may take the other side of a decision: its reprojected
    coordinates lie within `safety` times a first-order bound of their binary32 rounding error (in pixels) of a bound, a weight
    rounding step or a truncation step, or its distance lies within `margin_rel` of the cutoff.

    -> dict: rgb float64[h, w, 3], a float64[h, w] (next_blending); boolean masks sky, outside, rejected, accepted, behind (reprojected
    behind the old camera), edge (accepted with a weight exactly 0 or 1), fragile, cmp_rgb / cmp_a (the result is defined by the shader and the sampler rule); fy, ay: texel row coordinate and its weight."""
    h, w = color.shape[:2]
    f64 = np.float64
    col, n = color[..., :3].astype(f64), nd[..., :3].astype(f64)
    depth = nd[..., 3].astype(f64)
    c, oc = np.asarray(c16, f64), np.asarray(old_c16, f64)
    o, oo, orr, ou, of = c[0:3], oc[0:3], oc[4:7], oc[8:11], oc[12:15]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # a NaN or infinite depth makes old_screen NaN (0 * inf or inf / inf), so the bounds test below fails: blending 1
        world = o + depth[..., None] * pixel_dirs(c16, w, h)                          # :62-68
        # old_screen_to_world: columns right, up, forward, origin (:75-80); its inverse (:82)
        m = np.eye(4)
        m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = orr, ou, of, oo
        inv = np.linalg.inv(m)
        s = world @ inv[:3, :3].T + inv[:3, 3]                                        # :84
        sx, sy = s[..., 0] / s[..., 2], s[..., 1] / s[..., 2]                         # :85
        tx, ty = (sx + 0.5) * (1.0 / w), (sy - 0.5) * (-1.0 / h)                      # :88-89
        hit = depth >= 0                                                              # :74 (NaN: false)
        inside = hit & (0 <= tx) & (tx <= 1) & (0 <= ty) & (ty <= 1)                  # :92
        old_d, fx, fy, ax, ay = _sample(old_nd[..., 3:4].astype(f64), tx, ty, inside)  # :94-97
        old_d = old_d[..., 0]
        ix, iy = np.trunc(np.where(inside, sx + 0.5, 0.0)), np.trunc(np.where(inside, sy - 0.5, 0.0))   # int(): toward zero
        od = ix[..., None] * orr + iy[..., None] * ou + of                            # :99-103
        od = od / np.sqrt((od * od).sum(-1, keepdims=True))
        old_pos = oo + old_d[..., None] * od                                          # :104
        to_cam = o - world
        cam_dir = to_cam / np.sqrt((to_cam * to_cam).sum(-1, keepdims=True))          # :107
        # :109 max(0, dot): a NaN dot is the only undefined case, and either answer (0 or NaN) makes the compare below false
        bias = np.maximum(0.0, (cam_dir * n).sum(-1))
        dist = np.sqrt(((old_pos - world) ** 2).sum(-1))                              # :110
        thr = bias * tu.blending_distance_cutoff * depth
        accepted = inside & (dist < thr)                                              # :113-114
        old_c, *_ = _sample(old_color.astype(f64), tx, ty, accepted)                  # :116
        old_rgb = np.where(accepted[..., None], old_c[..., :3], 0.0)
        blending = np.where(accepted, old_c[..., 3], 1.0)                             # :117
        b = blending[..., None]
        rgb = np.where(hit[..., None], old_rgb * (1 - b) + col * b, col)               # :122 mix(x, y, a) = x (1 - a) + y a
        pre = (1 - tu.sample_blending) * blending                                     # :123
        a = np.clip(pre, 1 - tu.maximum_blending, 1)

        cmp_rgb = ~(hit & (np.isinf(col).any(-1) | np.isinf(old_rgb).any(-1) | np.isinf(blending)))
        cmp_a = ~np.isnan(pre)
        # fragile: a binary32 evaluation may take the other side of a boundary.  First-order rounding error of old_screen.xy in
        # pixels: each row of the matrix product, with the error world_pos already carries, then the perspective division.
        eps = 2.0 ** -24
        absinv = np.abs(inv[:3, :3])
        row_err = eps * (4 * np.abs(world) @ absinv.T + 2 * np.abs(inv[:3, 3]) + absinv.sum(-1) * (np.abs(o).max() + 2 * np.abs(depth))[..., None])
        az = np.abs(s[..., 2])
        margin_px = safety * ((row_err[..., 0] + np.abs(sx) * row_err[..., 2]) / az + 4 * eps * (np.abs(sx) + 1))
        margin_py = safety * ((row_err[..., 1] + np.abs(sy) * row_err[..., 2]) / az + 4 * eps * (np.abs(sy) + 1))
        near_bounds = hit & ((np.abs(tx * w) < margin_px) | (np.abs(tx * w - w) < margin_px) |
                             (np.abs(ty * h) < margin_py) | (np.abs(ty * h - h) < margin_py))
        near_weight = inside & (_near_int((fx - np.floor(fx)) * 256.0 + 0.5, margin_px * 256) |
                                _near_int((fy - np.floor(fy)) * 256.0 + 0.5, margin_py * 256))
        near_trunc = inside & (_near_int(sx + 0.5, margin_px) | _near_int(sy - 0.5, margin_py))
        scale = np.abs(world).max(-1) + np.abs(oo).max() + np.abs(old_d)
        near_dist = inside & (thr > 0) & (np.abs(dist - thr) < margin_rel * thr + 16 * eps * scale)
    fragile = (near_bounds | near_weight | near_trunc | near_dist) & ~np.isnan(sx) & ~np.isnan(sy)
    edge = accepted & ((ax == 0) | (ax == 1) | (ay == 0) | (ay == 1))
    return dict(rgb=rgb, a=a, sky=~hit, outside=hit & ~inside, behind=hit & (s[..., 2] < 0), rejected=inside & ~accepted, accepted=accepted, edge=edge,
                fragile=fragile, cmp_rgb=cmp_rgb, cmp_a=cmp_a, fy=fy, ay=ay)


def disagreement(got, ref, rtol=1e-5):
    """Pixels where a binary32 result (float32[h, w, 4]) and temporal_f64's `ref` disagree on comparable, non-fragile pixels:
    rgb and next_blending within rtol relative (NaN matches NaN, inf matches the same inf).  -> bool[h, w]."""
    def off(a, b, ok):
        with np.errstate(invalid="ignore"):
            close = (a == b) | (np.abs(a - b) <= rtol * np.maximum(np.abs(b), 1.0)) | (np.isnan(a) & np.isnan(b))
        return ok & ~close
    keep = ~ref["fragile"]
    return off(got[..., :3], ref["rgb"], (keep & ref["cmp_rgb"])[..., None]).any(-1) | off(got[..., 3], ref["a"], keep & ref["cmp_a"])
