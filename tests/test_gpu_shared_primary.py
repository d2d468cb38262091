"""VXRT_OPT_SHARED_PRIMARY (csrc/trace.hip: first_hit_kernel; csrc/trace_block.h): a trace launch whose frames all have one camera walks
each pixel's primary ray once, and every frame takes its first hit from that walk's record.  Nothing a frame holds may change:
every comparison here is bit for bit, option on against option off, and against the CPU oracle where a case says so."""
import numpy as np
import pytest

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

LABELS = ("colour", "nd", "albedo")


def _view(scenes, name, camera):
    pos, mrgb, size = scenes.load_scene(name)
    cam = {"bench": scenes.bench_camera, "close": scenes.close_camera}[camera](size)
    return pos, mrgb, cam


def _launch(H, noise, pos, mrgb, cam, w, h, batch, shared, bounces=3, tracer=0, rank=0, nranks=1, first_frame=1, accumulate=False):
    """One launch of `batch` frames (first_frame ..) in a fresh context -> (the last frame's three images [+ the colour accumulated
    over ALL the launch's frames by the temporal stage], rays of all frames, launches that shared, frame-lane launches, local rows)."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, TEMPORAL, TRACE, Camera, Context
    with Context(w, h, max_bounces=bounces, noise=noise, tracer=tracer, frames_per_launch=batch, frames_in_flight=2, rank=rank, nranks=nranks,
                 band_rows=8) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = Camera(*cam)
        ctx.set_option(H.OPT_SHARED_PRIMARY, shared)
        ctx.set_frame_number(first_frame - 1)
        ctx.render_frames(TRACE | TEMPORAL if accumulate else TRACE, batch)
        st = ctx.stats()
        imgs = [ctx.read(i) for i in range(3)] + ([ctx.read(ACCUM_COLOR)] if accumulate else [])
        return imgs, st.rays, ctx.shared_primary_launches(), st.frame_lane_launches, ctx.local_rows()


@pytest.mark.parametrize("w,h,nranks,rank,batch,tracer,name,camera,oracle", [
    (150, 70, 1, 0, 2, 0, "menger", "bench", False),
    (150, 70, 1, 0, 6, 0, "menger", "close", False),      # no multiple of 4: one frame per wave
    (150, 70, 1, 0, 8, 0, "menger", "close", True),
    (150, 70, 1, 0, 12, 0, "3x3x3", "bench", False),      # frame lanes of 4
    (150, 70, 1, 0, 16, 0, "menger", "bench", False),
    (150, 70, 3, 1, 16, 0, "menger", "close", False),
    (97, 41, 1, 0, 24, 1, "3x3x3", "close", False),
    (64, 48, 2, 1, 32, 4, "menger", "bench", False)])
def test_shared_primary_changes_nothing(O, H, scenes, noise, w, h, nranks, rank, batch, tracer, name, camera, oracle):
    """Option 1 against 0 for one launch: the three images of the launch's last frame, the ray total of all its frames and — on a
    single rank, where the temporal stage needs no neighbour — the colour that stage accumulates over EVERY frame of the launch (it
    reads each frame's colour and normal/depth in turn, so a difference in any frame shows) are identical.  Frame sizes that are no
    multiple of 8, row bands, launches with frame lanes of 8, of 4 and without, the all-in-one kernel and the head + tail pair."""
    pos, mrgb, cam = _view(scenes, name, camera)
    got = {s: _launch(H, noise, pos, mrgb, cam, w, h, batch, s, tracer=tracer, rank=rank, nranks=nranks, accumulate=nranks == 1) for s in (1, 0)}
    assert got[1][2] > 0 and got[0][2] == 0                                        # the launch shared / issued the launches of old
    assert got[1][3] == got[0][3] == (1 if batch % 4 == 0 else 0)                  # frame lanes are decided as before
    for a, b, label in zip(got[1][0], got[0][0], LABELS + ("accumulated colour of all frames",)):
        assert_bits_equal(a, b, f"{label}: shared primary rays on vs off, {name} {camera} x {batch}")
    assert got[1][1] == got[0][1]
    if oracle:
        u = O.Uniforms.default()
        u.set_camera(cam[0], O.camera_axis_scaled(cam[0], cam[1], cam[2], w, h))
        octree = O.create_octree(pos, mrgb)
        per_frame = [O.trace(octree, noise, (setattr(u, "frame_number", f) or u), w, h, 3, crop=(0, 0, w, h)) for f in range(1, batch + 1)]
        for a, b, label in zip(got[1][0], per_frame[-1][:3], LABELS):
            assert_bits_equal(a, b[got[1][4]], f"{label}: shared primary rays vs oracle")
        assert got[1][1] == sum(r[3] for r in per_frame)                           # every frame's primary ray is counted


def test_render_spp_with_the_gbuffer_mask(H, scenes, noise):
    """vxrt_render_spp(ALL, 4): four samples of one camera in one launch, of which only the kept one writes normal/depth and
    albedo/node — the displayed frame and the history it leaves are the same with the option on and off."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, ALL, DENOISED, Camera, Context
    pos, mrgb, cam = _view(scenes, "menger", "close")
    got = {}
    for shared in (1, 0):
        with Context(160, 96, max_bounces=3, noise=noise, frames_per_launch=4) as ctx:
            ctx.recreate_octree(pos, mrgb)
            ctx.camera = Camera(*cam)
            ctx.set_option(H.OPT_SHARED_PRIMARY, shared)
            frames = []
            for _ in range(2):                                                     # the second displayed frame blends with the first's history
                ctx.render_spp(ALL, 4)
                frames += [ctx.read(DENOISED), ctx.read(ACCUM_COLOR), ctx.read(1), ctx.read(2)]
            got[shared] = frames
            assert ctx.shared_primary_launches() == (2 if shared else 0)
    for i, (a, b) in enumerate(zip(got[1], got[0])):
        assert_bits_equal(a, b, f"render_spp image {i}: shared primary rays on vs off")


def test_render_path_shares_only_equal_cameras(H, scenes, noise):
    """vxrt_render_path: sharing is decided by comparing the launch's cameras.  Distinct poses: nothing is shared and every frame equals
    a vxrt_render of its own; identical poses: the launch shares, and its frames are what they are without the option."""
    from gpu_voxel_raytracer_amd import TRACE, Camera, Context
    pos, mrgb, cam = _view(scenes, "menger", "close")
    w, h, n = 128, 72, 8
    p0, d0 = np.asarray(cam[0], np.float32), np.asarray(cam[1], np.float32)
    side = np.cross(d0, np.array([0.0, 1.0, 0.0], np.float32)).astype(np.float32)
    moving = (np.stack([p0 + 0.05 * k * side for k in range(n)]).astype(np.float32), np.stack([d0] * n))
    still = (np.stack([p0] * n), np.stack([d0] * n))
    for count in (n, 3):                                                           # the last frame of a launch of `count` poses is frame `count`
        with Context(w, h, max_bounces=3, noise=noise, frames_per_launch=n) as ctx:
            ctx.recreate_octree(pos, mrgb)
            ctx.render_path(TRACE, moving[0][:count], moving[1][:count], cam[2])
            assert ctx.shared_primary_launches() == 0
            path = [ctx.read(i) for i in range(3)]
        with Context(w, h, max_bounces=3, noise=noise) as ctx:
            ctx.recreate_octree(pos, mrgb)
            ctx.camera = Camera(moving[0][count - 1], moving[1][count - 1], cam[2])
            ctx.set_frame_number(count - 1)
            ctx.render(TRACE)
            for i, label in enumerate(LABELS):
                assert_bits_equal(path[i], ctx.read(i), f"{label}: frame {count} of a moving path vs its own render")
    got = {}
    for shared in (1, 0):
        with Context(w, h, max_bounces=3, noise=noise, frames_per_launch=n) as ctx:
            ctx.recreate_octree(pos, mrgb)
            ctx.set_option(H.OPT_SHARED_PRIMARY, shared)
            ctx.render_path(TRACE, still[0], still[1], cam[2])
            assert ctx.shared_primary_launches() == shared
            got[shared] = [ctx.read(i) for i in range(3)] + [ctx.stats().rays]
    for i, label in enumerate(LABELS):
        assert_bits_equal(got[1][i], got[0][i], f"{label}: a path of identical poses, shared on vs off")
    assert got[1][3] == got[0][3]


def test_axis_camera_inside_the_root(O, H, scenes, noise):
    """A camera on integer coordinates inside the root cube looking exactly along + z: the centre pixels' rays have a zero direction
    component and take the shader's literal walk (NaN plane times and all) in first_hit_kernel as they do in trace_kernel."""
    pos, mrgb, _ = scenes.load_scene("8x8x8")
    f32 = np.float32
    cam = (np.array([1, 1, -3], f32), np.array([0, 0, 1], f32), 1.0)
    w, h, batch = 64, 64, 8
    got = {s: _launch(H, noise, pos, mrgb, cam, w, h, batch, s) for s in (1, 0)}
    assert got[1][2] == 1 and got[0][2] == 0
    u = O.Uniforms.default()
    u.set_camera(cam[0], O.camera_axis_scaled(cam[0], cam[1], cam[2], w, h))
    u.frame_number = batch
    ref = O.trace(O.create_octree(pos, mrgb), noise, u, w, h, 3, crop=(0, 0, w, h))
    assert np.isnan(ref[1][..., 3]).any() or np.isnan(ref[0]).any()                # the literal walk's NaNs really are in the frame
    for i, label in enumerate(LABELS):
        assert_bits_equal(got[1][0][i], got[0][0][i], f"{label}: axis camera, shared on vs off")
        assert_bits_equal(got[1][0][i], ref[i], f"{label}: axis camera vs oracle")
    assert got[1][1] == got[0][1]


def _cap_scene():
    """tests/test_gpu_trace.py: cap_scene — a row of 4 096 voxels along x (depth 12): a ray that runs along the row through the empty
    cells beside it is still inside the root cube when its 2 048th trip begins, and the walk returns the iteration cap's "hit"."""
    n = 4096
    pos = np.zeros((n, 3), np.int16)
    pos[:, 0] = np.arange(n)
    return pos, np.tile(np.array([[0, 200, 100, 50]], np.uint8), (n, 1))


def test_first_hits_at_the_iteration_cap(O, H, noise):
    """Hits that are no leaves: the cap's "hit" (node = the leaf bit alone, normal 0) goes through the record and comes out as it went
    in — hundreds of capped primary rays whose paths go on from there, equal to the oracle's."""
    pos, mrgb = _cap_scene()
    cam = (np.array([-1, 0.6, 0.25], np.float32), np.array([1, 0, 0], np.float32), 0.01)
    w, h, batch = 96, 64, 4
    got = {s: _launch(H, noise, pos, mrgb, cam, w, h, batch, s) for s in (1, 0)}
    assert got[1][2] == 1 and got[0][2] == 0
    u = O.Uniforms.default()
    u.set_camera(cam[0], O.camera_axis_scaled(cam[0], cam[1], cam[2], w, h))
    u.frame_number = batch
    ref = O.trace(O.create_octree(pos, mrgb), noise, u, w, h, 3, crop=(0, 0, w, h))
    capped = ref[2][..., 3].view(np.uint32) == 0x80000000
    assert capped.sum() > 500 and (ref[1][..., 3] >= 0).sum() > capped.sum() + 500   # capped and ordinary hits
    assert np.array_equal(got[1][0][2][..., 3].view(np.uint32) == 0x80000000, capped)
    for i, label in enumerate(LABELS):
        assert_bits_equal(got[1][0][i], got[0][0][i], f"{label}: capped rays, shared on vs off")
        assert_bits_equal(got[1][0][i], ref[i], f"{label}: capped rays vs oracle")
    assert got[1][1] == got[0][1]


def test_no_stale_first_hits(H, scenes, noise):
    """Nothing is kept from one launch to the next: after a voxel edit, and after a camera change, a context's next launch equals the
    same launch of a fresh context that never saw the earlier scene or camera."""
    from gpu_voxel_raytracer_amd import TRACE, Camera, Context
    pos, mrgb, cam = _view(scenes, "menger", "close")
    _, _, other = _view(scenes, "menger", "bench")
    w, h, batch = 150, 70, 8
    # the edit: every voxel of the lower half along x goes — the half this camera faces — except the plane x = min (the scene keeps its
    # extent, so a rebuild has the same root)
    x = pos[:, 0].astype(np.int32)
    gone = (x < (int(x.min()) + int(x.max())) // 2) & (x > int(x.min()))
    assert gone.any() and not gone.all()
    fresh_edit = _launch(H, noise, pos[~gone], mrgb[~gone], cam, w, h, batch, 1, first_frame=batch + 1)
    fresh_cam = _launch(H, noise, pos, mrgb, other, w, h, batch, 1, first_frame=batch + 1)
    for what, fresh in (("edit", fresh_edit), ("camera", fresh_cam)):
        with Context(w, h, max_bounces=3, noise=noise, frames_per_launch=batch) as ctx:   # one trace stream: both launches use ONE set of records
            ctx.recreate_octree(pos, mrgb)
            ctx.camera = Camera(*cam)
            ctx.render_frames(TRACE, batch)
            before = ctx.read(1)
            if what == "edit":
                ctx.clear_voxels(pos[gone])
            else:
                ctx.camera = Camera(*other)
            ctx.reset_stats()
            ctx.render_frames(TRACE, batch)
            after = [ctx.read(i) for i in range(3)]
            assert ctx.shared_primary_launches() == 1 and ctx.stats().rays == fresh[1]
        changed = (before[..., 3] != after[1][..., 3]).mean()
        assert changed > 0.05, (what, changed)                                     # the first hits really moved
        for i, label in enumerate(LABELS):
            assert_bits_equal(after[i], fresh[0][i], f"{label}: second launch after a {what} change vs a fresh context")
