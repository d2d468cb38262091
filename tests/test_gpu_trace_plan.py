"""Which launches a trace launch goes out as (csrc/api_trace.hip: plan_trace and the issuing functions behind trace_frames).  The parity
matrix (test_gpu_trace.py) pins images only: a change that stopped sharing the primary rays, stopped putting frames into a wave's lanes or
stopped splitting by priority would still be bit-exact.  Here the three counters that say what went out — vxrt_stats.frame_lane_launches,
vxrt_debug_shared_primary_launches, vxrt_stats.split_launches — are compared with what the rules give, launch by launch:

* frame lanes: the option on, the 8-byte records, whole groups of frames (8 | g or 4 | g), and along a camera path an estimated image
  motion of at most 16 pixels across every group; counted on every path that runs trace_kernel or fused_kernel (no scene here is
  beyond the Infinity Cache);
* shared primary rays: the option on, g >= 2, the 8-byte records, every camera of the launch equal to the first, not the fused kernel;
* priority split: the option on, a tile order for the launch's stream whose walking-tile count has reached the host (a stream's second
  launch onwards: every render call here is followed by a sync), some but not all tiles walking, and neither the fused kernel nor a
  launch that has its longest tiles apart.

The expected totals are summed from those rules, never recorded from a run.  Images and ray totals equal those of the same context
with the three options off: after the launches at rest, and again after the camera paths.

One comparison is narrower than that.  A head + tail launch that went out split by priority (_split_races: trace_kernel as two grids
followed by bounce_kernel or path_kernel) joins its low-priority grid only behind the tail, so a path that grid hands over — it has none
while the camera rests, its tiles store sky, but a moving camera brings geometry into them — races with the tail: it can be lost, or be followed
twice (seen on the commit that introduced this test: 315 318 .. 315 385 rays against 315 411 at g = 3, 803 145 against 803 057 at g = 8).  That is the experiment's defect
(-DVXRT_VARIANTS=1 builds only), older than this test and recorded in HISTORY.md.  For those launches alone the state AFTER THE CAMERA
PATHS is held to what the race cannot break: the normal / depth and albedo images (the head writes them, whichever grid) are bit-equal;
the colour and the ray total are not compared.  Every other launch — the all-in-one kernel split or not, the
fused kernel, the long tiles — is compared in full.

What the counters prove: they are counted from the launch's plan, so they pin what was DECIDED.  That the issuing functions launch
what the plan says is seen by the image and ray comparisons only where it changes a result; a share flag that launched no
first_hit_kernel would still be bit-exact.  The kernels that really go out are compared by scripts/trace_plan_launches.py under
rocprofv3 (profiles/trace_plan/kernel_counts.txt), not by this suite."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal, require_variants

pytestmark = pytest.mark.gpu

W, HH, BOUNCES = 128, 96, 3
GS = (1, 2, 3, 4, 8, 12)
# kind -> (vxrt_config.tracer with 0 = auto, wide records, fused tail, long tiles per mille)
KINDS = {"auto": (0, 0, 0, 0), "1": (1, 0, 0, 0), "4": (4, 0, 0, 0), "5": (5, 0, 0, 0), "wide": (0, 1, 0, 0), "fused": (4, 0, 1, 0),
         "long": (4, 0, 0, 100)}
SMALL, LARGE = 0.25, 20.0        # pixels of image motion per frame of the two camera paths: 1.75 and 140 across 8 frames, 0.75 and 60 across 4


def _focal_px(fov):
    return 0.5 * HH / np.tan(0.5 * float(fov))


def _rotating_path(cam, g, pixels_per_frame):
    """g poses at the camera's position, the direction turning about the y axis by `pixels_per_frame` of image motion per frame."""
    pos, d = np.asarray(cam[0], np.float64), np.asarray(cam[1], np.float64)
    dirs = []
    for k in range(g):
        t = k * pixels_per_frame / _focal_px(cam[2])
        dirs.append([np.cos(t) * d[0] + np.sin(t) * d[2], d[1], -np.sin(t) * d[0] + np.cos(t) * d[2]])
    return np.tile(pos, (g, 1)).astype(np.float32), np.asarray(dirs, np.float32)


def _group_motion(dirs, fov, lanes):
    """The largest image motion in pixels between the first and the last pose of any group of `lanes` frames (a pure rotation: angle x
    focal length)."""
    d = np.asarray(dirs, np.float64)
    worst = 0.0
    for k in range(0, len(d) - lanes + 1, lanes):
        a, b = d[k], d[k + lanes - 1]
        worst = max(worst, _focal_px(fov) * float(np.arccos(np.clip(a @ b / np.linalg.norm(a) / np.linalg.norm(b), -1, 1))))
    return worst


def _path(kind, g, inflight):
    """(the tracer that really runs: 0 all-in-one, 4 / 5 head + tail; the fused kernel runs; the longest tiles go apart) by the rules."""
    tracer, wide, fused, long_tiles = KINDS[kind]
    variant = {0: 4, 1: 0}.get(tracer, tracer)                    # the library's internal number
    effective = 0 if (tracer == 0 and g == 1 and inflight == 1) else variant
    fused_path = bool(fused) and effective == 4 and not wide      # the tail is one launch: from hit 1 of 3 bounces, no second queue below 6
    long_path = bool(long_tiles) and effective == 4 and not wide and not fused_path
    return effective, fused_path, long_path


def _split_races(kind, g, inflight, prio):
    """The launches are head + tail pairs whose head goes out split by priority: the low-priority grid may hand paths to a tail that
    has already started (the module's docstring)."""
    effective, fused_path, long_path = _path(kind, g, inflight)
    return bool(prio) and effective >= 4 and not fused_path and not long_path


def _expected(kind, g, inflight, shared, lanes, prio, launches, fov):
    """(frame-lane launches, shared launches, split launches) the rules give for `launches`: one entry per launch, in order — None for
    the camera at rest, the directions of the launch's poses for a camera path."""
    wide = KINDS[kind][1]
    effective, fused_path, long_path = _path(kind, g, inflight)
    want_lanes = (8 if g % 8 == 0 else 4 if g % 4 == 0 else 0) if (lanes and not wide) else 0
    n_lanes = n_shared = n_split = 0
    seen = set()
    for i, path in enumerate(launches):
        stream = i % inflight
        moving = path is not None and g > 1                        # one frame per launch: vxrt_render_path sets the camera and renders
        n_lanes += int(want_lanes != 0 and (not moving or _group_motion(path, fov, want_lanes) <= 16.0))
        n_shared += int(bool(shared) and g >= 2 and not wide and not fused_path and not moving)
        # a stream's first launch has no tile order yet; with the longest tiles apart every later one starts at a block > 0
        n_split += int(bool(prio) and stream in seen and not fused_path and not long_path)
        seen.add(stream)
    return n_lanes, n_shared, n_split


def _run(H, scenes, noise, kind, g, inflight, shared, lanes, prio):
    """Three launches of g frames at rest, then a camera path of small and one of large motion, a sync after every call ->
    ((images of the last frame, rays) after the launches at rest and after the paths, the three counters, the launches as _expected
    takes them, walking tiles, tiles, fov)."""
    from gpu_voxel_raytracer_amd import TRACE, Camera, Context
    pos, mrgb, size = scenes.load_scene("menger")
    cam = scenes.bench_camera(size)                               # from outside: the sponge in the middle, sky around it
    tracer, wide, fused, long_tiles = KINDS[kind]
    tuning = [(H.OPT_TAIL_CAPACITY, 4096), (H.OPT_SCENE_FORMAT, wide), (H.OPT_FUSED_TAIL, fused), (H.OPT_LONG_TILES, long_tiles),
              (H.OPT_TRACE_PRIORITY, prio), (H.OPT_SHARED_PRIMARY, shared), (H.OPT_FRAME_LANES, lanes)]
    with Context(W, HH, max_bounces=BOUNCES, noise=noise, tracer=tracer, frames_per_launch=g, frames_in_flight=inflight, tuning=tuning) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = Camera(*cam)
        launches = []
        for _ in range(3):
            ctx.render_frames(TRACE, g)
            ctx.sync()
            launches.append(None)
        at_rest = [ctx.read(i) for i in range(3)], ctx.stats().rays
        for step in (SMALL, LARGE):
            p, d = _rotating_path(cam, g, step)
            ctx.render_path(TRACE, p, d, cam[2])
            ctx.sync()
            launches.append(d)
        st = ctx.stats()
        order = np.zeros(((W + 7) // 8) * ((HH + 7) // 8), np.uint32)
        walking, spread = C.c_uint32(0), C.c_uint32(0)
        ctx._chk(ctx._L.vxrt_debug_tile_order(ctx._h, order.ctypes.data_as(C.c_void_p), None, C.c_size_t(order.size), C.byref(walking), C.byref(spread)), "tile order")
        imgs = [ctx.read(i) for i in range(3)]
        return (at_rest, (imgs, st.rays)), (st.frame_lane_launches, ctx.shared_primary_launches(), st.split_launches), launches, walking.value, order.size, cam[2]


CASES = ([(k, i, False) for k in ("auto", "1", "4") for i in (1, 2)] +                     # the product library: it holds no priority split
         [(k, i, True) for k in KINDS for i in (1, 2)])                                   # libvxrt_variants.so: every kind, priority off / on


@pytest.mark.parametrize("kind,inflight,variants", CASES)
def test_counters_follow_the_launch_rules(H, scenes, noise, kind, inflight, variants):
    if variants:
        require_variants(H, tracer=5)
    for g in GS:
        base = _run(H, scenes, noise, kind, g, inflight, 0, 0, 0)
        launches, fov = base[2], base[5]
        assert base[1] == (0, 0, 0), (kind, g, inflight, base[1])
        assert 0 < base[3] < base[4], "the view must hold tiles that walk and tiles of sky"
        if g % 4 == 0:                                                                     # the paths are far from the 16 pixels on either side
            assert _group_motion(launches[3], fov, 4) <= 4.0 and _group_motion(launches[4], fov, 4) >= 48.0
        for shared in (0, 1):
            for lanes in (0, 1):
                for prio in ((0, 1) if variants else (0,)):
                    if not (shared or lanes or prio):
                        continue
                    got = _run(H, scenes, noise, kind, g, inflight, shared, lanes, prio)
                    what = f"{kind} g={g} inflight={inflight} shared={shared} lanes={lanes} priority={prio}"
                    want = _expected(kind, g, inflight, shared, lanes, prio, launches, fov)
                    print(what, "counters (frame lanes, shared, split):", got[1], "expected", want)
                    assert got[1] == want, what
                    for when, mine, theirs in zip(("at rest", "after the camera paths"), got[0], base[0]):
                        racing = when != "at rest" and _split_races(kind, g, inflight, prio)
                        assert racing or mine[1] == theirs[1], f"{what}: rays {when}: {mine[1]} vs {theirs[1]}"
                        for a, b, label in list(zip(mine[0], theirs[0], ("colour", "nd", "albedo")))[1 if racing else 0:]:
                            assert_bits_equal(a, b, f"{label} {when}: {what} vs all three options off")
