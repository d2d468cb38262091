"""VXRT_OPT_SHARED_PRIMARY 2 (csrc/api_trace.hip: plan_trace, issue_head): the primary rays of one camera are walked once per API
call — a later launch of the call reads the records of the call's first walk, on another stream behind an event — and never kept
beyond the call.  Option 1 walks once per launch, option 0 never shares.  Nothing a frame holds may change: every comparison is bit
for bit between the three option values.  The shapes are small: what can go wrong are launch boundaries, the hand-over between
streams and ragged last launches, not the image size.  vxrt_debug_first_hit_walks counts the first_hit_kernel launches that really
went out, vxrt_debug_shared_primary_launches the launches that took their first hits from records."""
import numpy as np
import pytest

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

LABELS = ("colour", "nd", "albedo")
OPTIONS = (2, 1, 0)


def _view(scenes, name, camera):
    pos, mrgb, size = scenes.load_scene(name)
    cam = {"bench": scenes.bench_camera, "close": scenes.close_camera}[camera](size)
    return pos, mrgb, cam


def _context(H, noise, pos, mrgb, cam, w, h, option, batch, inflight=2, bounces=3, **kw):
    from gpu_voxel_raytracer_amd import Camera, Context
    ctx = Context(w, h, max_bounces=bounces, noise=noise, frames_per_launch=batch, frames_in_flight=inflight, **kw)
    try:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = Camera(*cam)
        if option is not None:
            ctx.set_option(H.OPT_SHARED_PRIMARY, option)
    except Exception:
        ctx.close()
        raise
    return ctx


def _images(ctx, extra=()):
    return [ctx.read(i) for i in (0, 1, 2) + tuple(extra)]


def _assert_same(got, what, labels=LABELS):
    """got[option] = (images, rays): options 1 and 0 against option 2."""
    for other in (1, 0):
        for a, b, label in zip(got[2][0], got[other][0], labels):
            assert_bits_equal(a, b, f"{label}: {what}, option 2 vs {other}")
        assert got[2][1] == got[other][1], (what, other, got[2][1], got[other][1])


@pytest.mark.parametrize("w,h,tracer,nranks,rank", [(150, 70, 0, 1, 0), (64, 48, 4, 1, 0), (150, 70, 0, 3, 1)])
def test_one_call_many_launches_two_streams(H, scenes, noise, w, h, tracer, nranks, rank):
    """render_frames(TRACE | TEMPORAL, 40) at 8 frames per launch on two streams: five launches, of which option 2 walks the first
    only — launches 1 and 3 read its records from the other stream.  The last frame's images, the colour the temporal stage
    accumulated over all 40 frames (it reads every frame in turn) and the ray total are those of options 1 and 0."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, TEMPORAL, TRACE
    pos, mrgb, cam = _view(scenes, "menger", "close")
    got = {}
    for option in OPTIONS:
        with _context(H, noise, pos, mrgb, cam, w, h, option, 8, tracer=tracer, nranks=nranks, rank=rank, band_rows=8) as ctx:
            ctx.render_frames(TRACE | TEMPORAL, 40)
            got[option] = (_images(ctx, (ACCUM_COLOR,)), ctx.stats().rays)
            assert ctx.first_hit_walks() == {2: 1, 1: 5, 0: 0}[option]
            assert ctx.shared_primary_launches() == (5 if option else 0)
    _assert_same(got, f"40 frames in 5 launches, tracer {tracer}, rank {rank} of {nranks}", LABELS + ("accumulated colour of all frames",))


@pytest.mark.parametrize("count,walks_per_launch", [(19, 3), (17, 2)])
def test_ragged_calls(H, scenes, noise, count, walks_per_launch):
    """19 frames are launches of 8 + 8 + 3 — the last without frame lanes, reading records a frame-lane launch's walk wrote; 17 are
    8 + 8 + 1, and a launch of one frame never shares.  One walk under option 2 either way."""
    from gpu_voxel_raytracer_amd import TRACE
    pos, mrgb, cam = _view(scenes, "menger", "close")
    got = {}
    for option in OPTIONS:
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 8) as ctx:
            ctx.render_frames(TRACE, count)
            got[option] = (_images(ctx), ctx.stats().rays)
            assert ctx.first_hit_walks() == {2: 1, 1: walks_per_launch, 0: 0}[option]
            assert ctx.shared_primary_launches() == (walks_per_launch if option else 0)
    _assert_same(got, f"a call of {count} frames at 8 per launch")


def test_render_spp_over_several_launches(H, scenes, noise):
    """render_spp(ALL, 12) at 4 frames per launch: three launches per displayed frame, the camera at rest; only the last launch's kept
    sample writes normal/depth and albedo.  Two displayed frames (the second blends with the first's history): one walk each."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, ALL, DENOISED
    pos, mrgb, cam = _view(scenes, "menger", "close")
    got = {}
    for option in OPTIONS:
        with _context(H, noise, pos, mrgb, cam, 160, 96, option, 4) as ctx:
            frames = []
            for _ in range(2):
                ctx.render_spp(ALL, 12)
                frames += [ctx.read(DENOISED), ctx.read(ACCUM_COLOR), ctx.read(1), ctx.read(2)]
            got[option] = (frames, ctx.stats().rays)
            assert ctx.first_hit_walks() == {2: 2, 1: 6, 0: 0}[option]
    names = tuple(f"{n} after displayed frame {f}" for f in (1, 2) for n in ("denoised", "accumulated colour", "nd", "albedo"))
    _assert_same(got, "render_spp of 12 samples at 4 per launch", names)


@pytest.mark.parametrize("what", ["edit", "camera", "nothing"])
def test_nothing_survives_a_call(H, scenes, noise, what):
    """Two calls of 24 frames (three launches each, two streams) with a voxel edit, a camera change or nothing between them: the second
    call walks again — two walks in all — and its last frame and its rays are those of a fresh context that never saw the first
    scene or camera."""
    from gpu_voxel_raytracer_amd import TRACE, Camera
    pos, mrgb, cam = _view(scenes, "menger", "close")
    _, _, other = _view(scenes, "menger", "bench")
    w, h, batch, frames = 150, 70, 8, 24
    # the edit of test_gpu_shared_primary.py: the half of the sponge this camera faces goes, except the plane that keeps the scene's extent
    x = pos[:, 0].astype(np.int32)
    gone = (x < (int(x.min()) + int(x.max())) // 2) & (x > int(x.min()))
    assert gone.any() and not gone.all()
    keep = ~gone if what == "edit" else np.ones(len(pos), bool)
    with _context(H, noise, pos[keep], mrgb[keep], other if what == "camera" else cam, w, h, 2, batch) as ctx:
        ctx.set_frame_number(frames)
        ctx.render_frames(TRACE, frames)
        fresh = (_images(ctx), ctx.stats().rays)
    with _context(H, noise, pos, mrgb, cam, w, h, 2, batch) as ctx:
        ctx.render_frames(TRACE, frames)
        before, rays_before = ctx.read(1), ctx.stats().rays
        assert ctx.first_hit_walks() == 1
        if what == "edit":
            ctx.clear_voxels(pos[gone])
        elif what == "camera":
            ctx.camera = Camera(*other)
        ctx.render_frames(TRACE, frames)
        after, rays = _images(ctx), ctx.stats().rays - rays_before
        assert ctx.first_hit_walks() == 2 and ctx.shared_primary_launches() == 6
    if what != "nothing":
        changed = (before[..., 3] != after[1][..., 3]).mean()
        assert changed > 0.05, (what, changed)                                     # the first hits really moved
    for a, b, label in zip(after, fresh[0], LABELS):
        assert_bits_equal(a, b, f"{label}: second call after {what} changed vs a fresh context")
    assert rays == fresh[1]


@pytest.mark.parametrize("batch", [12, 6])
def test_back_to_back_calls_with_different_cameras(H, scenes, noise, batch):
    """Call A (close view, 8 bounces: long launches) and, with no host sync between them, call B (bench view).  At 12 and at 6 frames
    per launch A is an even number of launches on two streams, so B's first launch runs on stream 0 and walks into the buffer that
    A's last launch, on stream 1, may still be reading: the walk waits for that launch's event (issue_head).  If it did not, A's
    first hits — and with them A's ray count — could move; a race does not show on every run, the ordering argument in issue_head is
    the proof and this the tripwire."""
    from gpu_voxel_raytracer_amd import TRACE, Camera
    pos, mrgb, cam_a = _view(scenes, "menger", "close")
    _, _, cam_b = _view(scenes, "menger", "bench")
    w, h, frames = 150, 70, 24
    with _context(H, noise, pos, mrgb, cam_a, w, h, 2, batch, bounces=8) as ctx:
        ctx.render_frames(TRACE, frames)
        rays_a = ctx.stats().rays
    with _context(H, noise, pos, mrgb, cam_b, w, h, 2, batch, bounces=8) as ctx:
        ctx.set_frame_number(frames)
        ctx.render_frames(TRACE, frames)
        alone_b = (_images(ctx), ctx.stats().rays)
    with _context(H, noise, pos, mrgb, cam_a, w, h, 2, batch, bounces=8) as ctx:
        ctx.render_frames(TRACE, frames)
        ctx.camera = Camera(*cam_b)
        ctx.render_frames(TRACE, frames)
        both = (_images(ctx), ctx.stats().rays)
        assert ctx.first_hit_walks() == 2
    assert both[1] == rays_a + alone_b[1], (both[1], rays_a, alone_b[1])
    for a, b, label in zip(both[0], alone_b[0], LABELS):
        assert_bits_equal(a, b, f"{label}: call B behind call A vs call B alone, {batch} frames per launch")


def test_render_path_walks_once_per_camera(H, scenes, noise):
    """vxrt_render_path: who called decides nothing, the cameras do.  24 identical poses at 8 per launch walk once under option 2 and
    give option 0's frames; 24 distinct poses neither walk nor share."""
    from gpu_voxel_raytracer_amd import TRACE
    pos, mrgb, cam = _view(scenes, "menger", "close")
    w, h, n = 128, 72, 24
    p0, d0 = np.asarray(cam[0], np.float32), np.asarray(cam[1], np.float32)
    side = np.cross(d0, np.array([0.0, 1.0, 0.0], np.float32)).astype(np.float32)
    still = (np.stack([p0] * n), np.stack([d0] * n))
    moving = (np.stack([p0 + 0.05 * k * side for k in range(n)]).astype(np.float32), np.stack([d0] * n))
    got = {}
    for option in (2, 0):
        with _context(H, noise, pos, mrgb, cam, w, h, option, 8) as ctx:
            ctx.render_path(TRACE, still[0], still[1], cam[2])
            got[option] = (_images(ctx), ctx.stats().rays)
            assert ctx.first_hit_walks() == (1 if option else 0) and ctx.shared_primary_launches() == (3 if option else 0)
    for a, b, label in zip(got[2][0], got[0][0], LABELS):
        assert_bits_equal(a, b, f"{label}: a path of 24 identical poses, option 2 vs 0")
    assert got[2][1] == got[0][1]
    with _context(H, noise, pos, mrgb, cam, w, h, 2, 8) as ctx:
        ctx.render_path(TRACE, moving[0], moving[1], cam[2])
        assert ctx.first_hit_walks() == 0 and ctx.shared_primary_launches() == 0
