"""VXRT_OPT_SKY_ONCE (csrc/api_trace.hip: plan_trace, settle_thin, refresh_walk_list; csrc/trace.hip: first_hit_kernel, walk_list_kernel):
inside one API call, a launch whose ring slots all hold the call's sky already runs trace_kernel over the tiles that walk alone.
Nothing a frame holds may change, and no ray may go uncounted: every comparison is bit for bit between option 1 and option 0 of one
library — the three images, the accumulated colour where the temporal stage ran, vxrt_stats.rays as an integer.  The shapes are small:
what can go wrong are ragged tiles, the ring's wrap, launch boundaries, the hand-over between streams and calls, not the image size.
vxrt_debug_thin_launches counts the launches that left tiles out, vxrt_debug_trace_blocks the blocks of trace_kernel that went out.

The scene is menger.  150 x 70 has a ragged right edge and ragged last rows, 100 x 75 has both edges ragged; through
scenes.bench_camera about three quarters of their tiles are all sky.  How many exactly is taken from a source the option does not
touch: the cost map of an option-0 run, in which trace_block itself notes a tile none of whose waves walked (kLightCost = 1)."""
import numpy as np
import pytest

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

LABELS = ("colour", "nd", "albedo")


def _tiles(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


def _sky_tiles(H, ctx, w, h):
    """Tiles of the whole-frame context whose cost-map entry is 1: no wave of theirs walked in the launches before the stream's last sort."""
    import ctypes as C
    n = _tiles(w, h)
    cost = np.zeros(n, np.uint32)
    walking, spread = C.c_uint32(0), C.c_uint32(0)
    H._check(H.lib().vxrt_debug_tile_order(ctx._h, None, cost.ctypes.data_as(C.c_void_p), C.c_size_t(n), C.byref(walking), C.byref(spread)),
             "vxrt_debug_tile_order")
    assert ((cost == 1) | (cost >= 4)).all() and walking.value == int((cost >= 4).sum())
    return int((cost == 1).sum())


def _view(scenes, camera="bench"):
    pos, mrgb, size = scenes.load_scene("menger")
    p, d, fov = {"bench": scenes.bench_camera, "close": scenes.close_camera, "away": scenes.bench_camera}[camera](size)
    if camera == "away":
        d = (-np.asarray(d, np.float32)).astype(np.float32)
    return pos, mrgb, (p, d, fov)


def _context(H, noise, pos, mrgb, cam, w, h, option, batch, inflight=2, bounces=3, **kw):
    from gpu_voxel_raytracer_amd import Camera, Context
    ctx = Context(w, h, max_bounces=bounces, noise=noise, frames_per_launch=batch, frames_in_flight=inflight, **kw)
    try:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = Camera(*cam)
        ctx.set_option(H.OPT_SKY_ONCE, option)
    except Exception:
        ctx.close()
        raise
    return ctx


def _images(ctx, extra=()):
    return [ctx.read(i) for i in (0, 1, 2) + tuple(extra)]


def _assert_same(on, off, what, labels=LABELS):
    """(images, rays) under option 1 against option 0."""
    for a, b, label in zip(on[0], off[0], labels):
        assert_bits_equal(a, b, f"{label}: {what}, sky once 1 vs 0")
    assert on[1] == off[1], (what, on[1], off[1])


@pytest.mark.parametrize("temporal", [False, True])
@pytest.mark.parametrize("tracer", [0, 4])
@pytest.mark.parametrize("w,h", [(150, 70), (100, 75)])
def test_slots_come_round(H, scenes, noise, w, h, tracer, temporal):
    """60 frames at 4 per launch, 2 in flight: 15 launches over a ring of 10 slots.  Launches 0 and 1 fill fresh slots, launch 2
    straddles the wrap (two of its slots are fresh): full.  From launch 3 on every slot holds the call's sky.  With the temporal
    stage the ring skips the history slot, which moves with every frame."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, TEMPORAL, TRACE
    pos, mrgb, cam = _view(scenes)
    tiles, sky_tiles = _tiles(w, h), None
    flags, extra = (TRACE | TEMPORAL, (ACCUM_COLOR,)) if temporal else (TRACE, ())
    got = {}
    for option in (0, 1):
        with _context(H, noise, pos, mrgb, cam, w, h, option, 4, tracer=tracer) as ctx:
            ctx.render_frames(flags, 60)
            got[option] = (_images(ctx, extra), ctx.stats().rays)
            thin, blocks = ctx.thin_launches(), ctx.trace_blocks()
            print(f"{w}x{h} tracer {tracer} temporal {temporal} option {option}: thin launches {thin}, trace blocks {blocks}")
            if option == 0:
                assert thin == 0 and blocks == 15 * tiles * 4
                sky_tiles = _sky_tiles(H, ctx, w, h)
                assert tiles // 2 < sky_tiles < tiles
            else:
                assert thin > 0
                assert thin == 12 or temporal               # without the moving history slot: every launch from the third on
                assert blocks == (15 - thin) * tiles * 4 + thin * (tiles - sky_tiles) * 4
    _assert_same(got[1], got[0], f"60 frames at {w}x{h}, tracer {tracer}", LABELS + ("accumulated colour of all frames",))


@pytest.mark.parametrize("frames", list(range(41, 51)))
def test_every_slot_is_looked_at(H, scenes, noise, frames):
    """The same call with 41 .. 50 frames: the slot that is current at the end — the one the images are read from — is each of the
    ring's ten in turn, written last by a thin launch, by a ragged one, or by a launch of one frame."""
    from gpu_voxel_raytracer_amd import TRACE
    pos, mrgb, cam = _view(scenes)
    got = {}
    for option in (1, 0):
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 4) as ctx:
            ctx.render_frames(TRACE, frames)
            got[option] = (_images(ctx), ctx.stats().rays)
            assert (ctx.thin_launches() > 0) == (option == 1)
    _assert_same(got[1], got[0], f"a call of {frames} frames")


@pytest.mark.parametrize("frames,thin", [(19, 0), (20, 2)])
def test_twice_round_the_ring(H, scenes, noise, frames, thin):
    """4 per launch, 2 in flight (ring 10).  A call of fewer than 2 x 10 frames asks for no flags and no list and issues the full
    launches throughout, although its last launches come back to slots it has written; 20 frames are five launches — two into fresh
    slots, the straddling one, two thin."""
    from gpu_voxel_raytracer_amd import TRACE
    pos, mrgb, cam = _view(scenes)
    tiles = _tiles(150, 70)
    got = {}
    for option in (1, 0):
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 4) as ctx:
            ctx.render_frames(TRACE, frames)
            got[option] = (_images(ctx), ctx.stats().rays)
            assert ctx.thin_launches() == (thin if option else 0)
            assert (ctx.trace_blocks() == tiles * frames) == (option == 0 or thin == 0)
    _assert_same(got[1], got[0], f"a call of {frames} frames over a ring of 10")


@pytest.mark.parametrize("frames", [43, 41])
def test_ragged_calls(H, scenes, noise, frames):
    """8 per launch (ring 18): 43 frames end in a launch of 3, which may be thin; 41 in a launch of one frame, which never shares and
    so is never thin: the blocks that thin launches left out are whole launches of 8 frames there."""
    from gpu_voxel_raytracer_amd import TRACE
    pos, mrgb, cam = _view(scenes)
    tiles, sky_tiles = _tiles(150, 70), None
    got, blocks, thin = {}, {}, {}
    for option in (0, 1):
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 8) as ctx:
            ctx.render_frames(TRACE, frames)
            got[option] = (_images(ctx), ctx.stats().rays)
            blocks[option], thin[option] = ctx.trace_blocks(), ctx.thin_launches()
            if option == 0:
                sky_tiles = _sky_tiles(H, ctx, 150, 70)
    print(f"{frames} frames: thin launches {thin}, trace blocks {blocks}")
    assert thin[0] == 0 and thin[1] > 0 and blocks[0] == tiles * frames
    left_out = blocks[0] - blocks[1]
    assert left_out % sky_tiles == 0
    thin_frames = left_out // sky_tiles
    assert thin_frames in ((8 * thin[1],) if frames == 41 else (8 * thin[1], 8 * (thin[1] - 1) + 3)), (thin_frames, thin[1])
    _assert_same(got[1], got[0], f"a call of {frames} frames at 8 per launch")


def test_gbuffer_bit(H, scenes, noise):
    """render_spp(ALL, 24) at 4 per launch: six launches per displayed frame.  The first five store colour only, so the slots are
    stamped without the G-buffer images; the last launch wants normal/depth and albedo of its kept sample and must go out full."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, ALL, DENOISED
    pos, mrgb, cam = _view(scenes)
    got = {}
    for option in (1, 0):
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 4) as ctx:
            frames = []
            for _ in range(2):
                ctx.render_spp(ALL, 24)
                frames += [ctx.read(DENOISED), ctx.read(ACCUM_COLOR), ctx.read(0), ctx.read(1), ctx.read(2)]
            got[option] = (frames, ctx.stats().rays)
            thin = ctx.thin_launches()
            print(f"render_spp, option {option}: thin launches {thin}")
            assert (0 < thin <= 2 * 2) if option else thin == 0    # launches 3 and 4 of each displayed frame at the most; never the last
    names = tuple(f"{n} after displayed frame {f}" for f in (1, 2) for n in ("denoised", "accumulated colour", "colour", "nd", "albedo"))
    _assert_same(got[1], got[0], "render_spp of 24 samples at 4 per launch", names)


@pytest.mark.parametrize("what", ["nothing", "camera", "sky", "edit"])
def test_nothing_survives_a_call(H, scenes, noise, what):
    """Two calls of 60 frames with, between them, nothing, a camera change that turns all-sky tiles into walking ones, a change of the
    sky's colour, or a voxel edit that grows the cull box.  The second call's frames and rays are those of a fresh context that made
    only that call, and its first three launches are full again: no slot's tag outlives the call that set it."""
    from gpu_voxel_raytracer_amd import TRACE, Camera
    pos, mrgb, cam = _view(scenes)
    _, _, close = _view(scenes, "close")
    w, h, frames = 150, 70, 60
    far = (pos.max(axis=0).astype(np.int32) + 24).astype(np.int16).reshape(1, 3)     # a voxel well outside the sponge: the cull box grows
    far_mrgb = np.array([[1, 200, 60, 60]], np.uint8)

    def change(ctx):
        if what == "camera":
            ctx.camera = Camera(*close)
        elif what == "sky":
            ctx.uniforms.sky_color[0], ctx.uniforms.sky_color[1], ctx.uniforms.sky_color[2] = 0.9, 0.3, 0.1
            ctx.uniforms.sun_strength = 3.0
        elif what == "edit":
            ctx.edit_voxels(far, far_mrgb, grow=True)

    with _context(H, noise, pos, mrgb, cam, w, h, 1, 4) as ctx:
        change(ctx)
        ctx.set_frame_number(frames)
        ctx.render_frames(TRACE, frames)
        fresh = (_images(ctx), ctx.stats().rays)
    with _context(H, noise, pos, mrgb, cam, w, h, 1, 4) as ctx:
        ctx.render_frames(TRACE, frames)
        before, rays_before, thin_before = ctx.read(0), ctx.stats().rays, ctx.thin_launches()
        box_before = ctx.culled_pixels()
        change(ctx)
        if what == "edit":
            assert ctx.culled_pixels() < box_before                                  # the box really grew
        ctx.render_frames(TRACE, frames)
        after, rays = _images(ctx), ctx.stats().rays - rays_before
        thin = ctx.thin_launches() - thin_before
    print(f"after {what}: thin launches {thin_before} in the first call, {thin} in the second")
    assert thin_before == 12 and 0 < thin <= 12
    if what != "nothing":
        assert (before != after[0]).any(axis=-1).mean() > 0.05, what                 # the frames really changed
    for a, b, label in zip(after, fresh[0], LABELS):
        assert_bits_equal(a, b, f"{label}: second call after {what} changed vs a fresh context")
    assert rays == fresh[1]


def test_back_to_back_calls_without_a_host_sync(H, scenes, noise):
    """Call A (bench view) and at once call B (close view): B's walk, flags and lists are issued while A's last launches are in
    flight, and B's first launch writes slots that A's tags still describe.  Both options give the same frames and rays."""
    from gpu_voxel_raytracer_amd import TRACE, Camera
    pos, mrgb, cam = _view(scenes)
    _, _, close = _view(scenes, "close")
    got = {}
    for option in (1, 0):
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 4, bounces=8) as ctx:
            ctx.render_frames(TRACE, 60)
            ctx.camera = Camera(*close)
            ctx.render_frames(TRACE, 60)
            got[option] = (_images(ctx), ctx.stats().rays)
            assert (ctx.thin_launches() > 12) == (option == 1)                        # both calls had thin launches
    _assert_same(got[1], got[0], "two calls back to back")


@pytest.mark.parametrize("camera", ["away", "close"])
def test_views_at_the_ends(H, scenes, noise, camera):
    """The camera turned away from the scene: every tile is sky, no launch is thin (a launch without a block would leave the tail's
    counter rotation behind), and 60 frames of tracer 4 are right all the same.  The close view: a few tiles of sky."""
    from gpu_voxel_raytracer_amd import TRACE
    pos, mrgb, cam = _view(scenes, camera)
    tiles, sky_tiles = _tiles(150, 70), None
    got = {}
    for option in (0, 1):
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 4, tracer=4) as ctx:
            ctx.render_frames(TRACE, 60)
            got[option] = (_images(ctx), ctx.stats().rays)
            thin, blocks = ctx.thin_launches(), ctx.trace_blocks()
            print(f"{camera} view, option {option}: thin launches {thin}, trace blocks {blocks}")
            if option == 0:
                sky_tiles = _sky_tiles(H, ctx, 150, 70)
                assert sky_tiles == tiles if camera == "away" else 0 < sky_tiles < tiles // 4
            if option == 0 or sky_tiles == tiles:
                assert thin == 0 and blocks == 15 * tiles * 4
            else:
                assert thin == 12 and blocks == (15 - thin) * tiles * 4 + thin * (tiles - sky_tiles) * 4
    if camera == "away":
        assert (got[1][0][1][..., 3] == -1.0).all() and got[1][1] == 60 * 150 * 70   # sky everywhere; one primary ray per pixel and frame
    _assert_same(got[1], got[0], f"the {camera} view")


@pytest.mark.parametrize("band_rows,tracer", [(8, 4), (4, 0)])
def test_bands(H, scenes, noise, band_rows, tracer):
    """Rank 1 of 3: the rank's tiles are 8 local rows, which at 4 rows per band come from two bands of the frame."""
    from gpu_voxel_raytracer_amd import TRACE
    pos, mrgb, cam = _view(scenes)
    got = {}
    for option in (1, 0):
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 4, tracer=tracer, nranks=3, rank=1, band_rows=band_rows) as ctx:
            ctx.render_frames(TRACE, 60)
            got[option] = (_images(ctx), ctx.stats().rays)
            print(f"band_rows {band_rows}, option {option}: thin launches {ctx.thin_launches()}, trace blocks {ctx.trace_blocks()}")
            assert (ctx.thin_launches() > 0) == (option == 1)
    _assert_same(got[1], got[0], f"rank 1 of 3 at {band_rows} rows per band")


def test_resort_inside_a_call(H, scenes, noise):
    """140 frames at 4 per launch: 35 launches on two streams, each of which sorts its tiles after its first launch and again after
    its 9th and 17th.  The list of walking tiles is cut again behind every sort, so every launch from the third on is thin."""
    from gpu_voxel_raytracer_amd import TRACE
    pos, mrgb, cam = _view(scenes)
    got = {}
    for option in (1, 0):
        with _context(H, noise, pos, mrgb, cam, 150, 70, option, 4, tracer=4) as ctx:
            ctx.render_frames(TRACE, 140)
            got[option] = (_images(ctx), ctx.stats().rays)
            assert ctx.thin_launches() == (32 if option else 0)
    _assert_same(got[1], got[0], "140 frames in 35 launches")
