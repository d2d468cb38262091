"""GPU: the temporal stage (csrc/post.hip: temporal_kernel, shaders/temporal.comp:48-125) on SYNTHETIC history under camera motion,
written straight into the context's images (tests/temporal_model.py builds it): NaN / inf colours and blending factors off the
1, 1/2, 1/4, ... ladder in the history, sky / zero / NaN / inf depths and odd normals in the current frame, reprojections that land on
texel centres (a texel of weight 0 must not be read), leave the view or fall behind the old camera.  Every case is bit-exact against
the oracle and agrees with the float64 model on its comparable, non-fragile pixels, for the temporal parameters across the GUI's
range, the fused radius-0 denoise, a traced pipeline whose parameters change between calls, and row bands whose history crosses
band edges through the halo.

Harness: after TRACE | TEMPORAL at the old camera, ACCUM_COLOR is accum[last] and NORMAL_DEPTH the slot that becomes the history
(csrc/api_context.hip: image_ptr, csrc/api_frame.hip: post_stages); the next trace goes to another slot of the ring (at least 3 slots:
alloc_images; trace_frames skips the history slot), so both stay the history of the TEMPORAL stage run after it."""
import ctypes as C

import numpy as np
import pytest

import temporal_model as M
from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

# (sample_blending, maximum_blending, blending_distance_cutoff): the defaults and corners of the GUI's ranges (src/context.rs:1778-1785)
PARAMS = [(0.5, 0.98, 1e-2), (0.0, 0.98, 1e-2), (1.0, 1.0, 1e-2), (0.25, 0.5, 1.0), (0.5, 0.0, 1e-4), (0.5, 0.98, 0.0)]


def hip():
    lib = C.CDLL("libamdhip64.so")
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    lib.hipFree.argtypes = [C.c_void_p]
    return lib


def put(rt, ctx, which, img):
    ptr, nbytes = ctx.device_image(which)
    img = np.ascontiguousarray(img, np.float32)
    assert nbytes == img.nbytes, (which, nbytes, img.nbytes)
    assert rt.hipMemcpy(C.c_void_p(ptr), img.ctypes.data_as(C.c_void_p), nbytes, 1) == 0


def set_params(ctx, p, albedo_factor=1.0):
    ctx.temporal_uniforms.sample_blending, ctx.temporal_uniforms.maximum_blending, ctx.temporal_uniforms.blending_distance_cutoff = p
    ctx.denoise_uniforms.radius = 0
    ctx.denoise_uniforms.albedo_factor = albedo_factor


def inject(rt, ctx, f, p, albedo_factor=1.0, rows=None, history=True, current=True):
    """Steps 1-4 of the harness on one context: the history of frame `f` at its old camera, then its current frame at the new one.
    rows: this rank's frame rows (band contexts)."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, ALBEDO_NODE, NORMAL_DEPTH, SAMPLED_COLOR, TEMPORAL, TRACE, Camera
    rr = slice(None) if rows is None else rows
    if history:
        ctx.camera = Camera(*f["old"])
        ctx.render(TRACE | TEMPORAL)
        ctx.sync()
        put(rt, ctx, ACCUM_COLOR, f["old_color"][rr])
        put(rt, ctx, NORMAL_DEPTH, f["old_nd"][rr])
    if current:
        ctx.camera = Camera(*f["new"])
        set_params(ctx, p, albedo_factor)
        ctx.render(TRACE)
        ctx.sync()
        for which, key in ((SAMPLED_COLOR, "color"), (NORMAL_DEPTH, "nd"), (ALBEDO_NODE, "alb")):
            put(rt, ctx, which, f[key][rr])
        ctx.update_bindings()


def oracle_temporal(O, f, p):
    return O.temporal(f["color"], f["nd"], f["old_color"], f["old_nd"], f["cam"], f["old_cam"], O.Temporal(*p), True)


def model(f, p):
    class T:
        sample_blending, maximum_blending, blending_distance_cutoff = p
    return M.temporal_f64(f["color"], f["nd"], f["old_color"], f["old_nd"], f["cam"], f["old_cam"], T)


def new_context(H, scenes, noise, w, h, **kw):
    from gpu_voxel_raytracer_amd import Context
    pos, mrgb, _ = scenes.load_scene("8x8x8")
    ctx = Context(w, h, max_bounces=1, noise=noise, frames_in_flight=kw.pop("frames_in_flight", 1), **kw)
    ctx.recreate_octree(pos, mrgb)
    return ctx


@pytest.mark.parametrize("w,h", [(65, 67), (130, 3), (97, 33), (256, 144), (1, 1), (2, 3)])
def test_temporal_equals_the_oracle_on_synthetic_history(O, H, scenes, noise, w, h):
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, TEMPORAL, Camera
    rt = hip()
    reached = {k: 0 for k in ("accepted", "rejected", "outside", "edge", "nan")}
    with new_context(H, scenes, noise, w, h) as ctx:
        for mi, motion in enumerate(M.MOTIONS):
            f = M.synthetic_frames(O, w, h, motion, seed=w * 1000 + h * 10 + mi)
            for cam, key in ((f["old"], "old_cam"), (f["new"], "cam")):     # the library's camera basis is the one the inputs assume
                r, u, fw = Camera(*cam).axis_scaled(w, h)
                assert np.array_equal(np.concatenate([r, u, fw]), np.concatenate([f[key][4:7], f[key][8:11], f[key][12:15]]))
            for p in PARAMS:
                inject(rt, ctx, f, p)
                ctx.render_stage(TEMPORAL)
                got = ctx.read(ACCUM_COLOR)
                assert_bits_equal(got, oracle_temporal(O, f, p), f"{w}x{h} {motion} {p}")
                ref = model(f, p)
                bad = M.disagreement(got, ref)
                assert not bad.any(), f"{w}x{h} {motion} {p}: {int(bad.sum())} pixels differ from the float64 model"
                for k in ("accepted", "rejected", "outside", "edge"):
                    reached[k] += int(ref[k].sum())
                reached["nan"] += int((ref["accepted"] & np.isnan(got[..., :3]).any(-1)).sum())
    if w * h >= 2000:
        assert all(v > 0 for v in reached.values()), reached


def test_zero_weight_texels_are_not_read_on_the_gpu(O, H, scenes, noise):
    """NaN in every other history texel: reprojections on texel centres (camera at rest) read only their own texel, so the texels
    between the NaNs stay finite; under a sub-pixel drift the NaNs carry weight and must show."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, TEMPORAL
    w, h = 64, 48
    rt = hip()
    with new_context(H, scenes, noise, w, h) as ctx:
        for motion in ("rest", "pixel_pan", "drift"):
            f = M.synthetic_frames(O, w, h, motion, seed=7, exotic=False)
            f["old_color"][::2, ::2, :3] = np.nan
            p = (0.5, 0.98, 1e-2)
            inject(rt, ctx, f, p)
            ctx.render_stage(TEMPORAL)
            got = ctx.read(ACCUM_COLOR)
            assert_bits_equal(got, oracle_temporal(O, f, p), motion)
            ref = model(f, p)
            assert not M.disagreement(got, ref).any(), motion
            exact = ref["accepted"] & (ref["edge"] if motion != "drift" else ~ref["edge"])
            assert exact.sum() > 100, motion
            nan = np.isnan(got[exact][:, :3]).any(-1)
            if motion == "drift":
                assert nan.mean() > 0.5
            else:
                assert 0.1 < nan.mean() < 0.5                  # a quarter of the texels are NaN, and only those show


@pytest.mark.parametrize("albedo_factor", [0.0, 0.37, 1.0])
def test_fused_radius0_denoise_after_synthetic_temporal(O, H, scenes, noise, albedo_factor):
    """TEMPORAL | DENOISE at radius 0 is one fused launch (csrc/post.hip: temporal_kernel with albedo); TEMPORAL then DENOISE is two.
    Both give O.denoise(O.temporal(...)) bit for bit, for the albedo factors the GUI offers."""
    from gpu_voxel_raytracer_amd import DENOISE, DENOISED, TEMPORAL
    w, h = 97, 33
    rt = hip()
    with new_context(H, scenes, noise, w, h) as ctx:
        for motion in ("drift", "rotation", "rest"):
            f = M.synthetic_frames(O, w, h, motion, seed=int(albedo_factor * 100) + len(motion))
            p = (0.25, 0.5, 1.0)
            du = O.Denoise.default()
            du.radius, du.albedo_factor = 0, albedo_factor
            want = O.denoise(oracle_temporal(O, f, p), f["nd"], f["alb"], f["cam"], du)
            assert np.isfinite(want[..., :3]).mean() > 0.8
            inject(rt, ctx, f, p, albedo_factor)
            ctx.render_stage(TEMPORAL | DENOISE)
            assert_bits_equal(ctx.read(DENOISED), want, f"fused, {motion}, albedo factor {albedo_factor}")
            inject(rt, ctx, f, p, albedo_factor)
            ctx.render_stage(TEMPORAL)
            ctx.render_stage(DENOISE)
            assert_bits_equal(ctx.read(DENOISED), want, f"separate launches, {motion}, albedo factor {albedo_factor}")


# per call: temporal parameters and number of frames (render_path: rounded up to whole batches of 4); the last call reaches the
# floor 1 - maximum_blending of next_blending
SCHEDULE = [((0.5, 0.98, 1e-2), 2), ((0.25, 0.5, 1.0), 3), ((0.5, 0.9, 0.0), 1), ((0.0, 0.98, 1e-2), 1), ((1.0, 1.0, 1e-2), 1),
            ((0.5, 0.0, 1e-4), 2), ((0.5, 0.98, 0.05), 7)]


@pytest.mark.parametrize("inflight,batch,radius", [(2, 1, 0), (3, 1, 1), (2, 4, 0)])
def test_temporal_parameters_change_between_calls_in_the_pipeline(O, H, scenes, noise, inflight, batch, radius):
    """A traced castle with a drifting camera; temporal_uniforms change between calls (render, or render_path batches of 4 frames
    per trace launch).  ACCUM_COLOR and DENOISED after each call equal an oracle loop that uses the same parameters per call."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, ALL, DENOISED, Camera, Context
    w, h, bounces = 72, 48, 2
    pos, mrgb, size = scenes.load_scene("castle")
    p0, d0, fov = scenes.close_camera(size)
    step = np.float32(0.0005 * float(max(size))) * np.array([1.0, 0.3, 0.0], np.float32)
    octree = O.create_octree(pos, mrgb)
    u = O.Uniforms.default()
    du = O.Denoise.default()
    du.radius = radius
    old_c, old_nd, old_cam = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), np.zeros(16, np.float32)
    frame = 0
    with Context(w, h, max_bounces=bounces, noise=noise, frames_in_flight=inflight, frames_per_launch=batch) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.denoise_uniforms.radius = radius
        for p, n in SCHEDULE:
            n = n if batch == 1 else 4 * ((n + 3) // 4)
            ctx.temporal_uniforms.sample_blending, ctx.temporal_uniforms.maximum_blending, ctx.temporal_uniforms.blending_distance_cutoff = p
            poses = [((p0 + (frame + k) * step).astype(np.float32), d0) for k in range(n)]
            if batch == 1:
                for cp, cd in poses:
                    ctx.camera = Camera(cp, cd, fov)
                    ctx.render(ALL)
            else:
                ctx.render_path(ALL, [q[0] for q in poses], [q[1] for q in poses], fov)
            for cp, cd in poses:
                frame += 1
                u.frame_number = frame
                u.set_camera(cp, O.camera_axis_scaled(cp, cd, fov, w, h))
                cam16 = u.camera16()
                color, nd, alb, _ = O.trace(octree, noise, u, w, h, bounces, crop=(0, 0, w, h))
                accum = O.temporal(color, nd, old_c, old_nd, cam16, old_cam, O.Temporal(*p), frame > 1)
                old_c, old_nd, old_cam = accum, nd, cam16
            assert_bits_equal(ctx.read(ACCUM_COLOR), accum, f"accumulated colour after frame {frame}, params {p}")
            assert_bits_equal(ctx.read(DENOISED), O.denoise(accum, nd, alb, cam16, du), f"denoised after frame {frame}, params {p}")
    assert frame >= 8
    hit = nd[..., 3] >= 0
    assert hit.mean() > 0.3
    assert np.isclose(accum[..., 3][hit], 0.02).mean() > 0.5          # the (1 - 0.98) floor of next_blending is reached


@pytest.mark.parametrize("nranks,band,motion", [(2, 16, "rotation"), (3, 32, "pixel_pan"), (2, 32, "drift"), (3, 16, "rotation")])
def test_synthetic_history_across_band_edges(O, H, scenes, noise, nranks, band, motion):
    """Row bands: exotic history in the rows either side of every band edge, read through the halo (csrc/post.hip: history_texel
    rebuilds the colour texel's .a from its own channel and the depth from .w).  The stitched ACCUM_COLOR equals the single-frame
    oracle, and some accepted pixels really read a neighbour's rows."""
    from gpu_voxel_raytracer_amd import ACCUM_COLOR, TEMPORAL, Camera
    from gpu_voxel_raytracer_amd.host import OPT_HALO_ROWS
    w, h = 96, 200
    rng = np.random.default_rng(nranks * 100 + band)
    f = M.synthetic_frames(O, w, h, motion, seed=nranks * 10 + band)
    for y in range(band, h, band):                                # salt the rows either side of each band edge
        for yy in (y - 2, y - 1, y, y + 1):
            cols = rng.random(w)
            f["old_color"][yy, cols < 0.15, 3] = M.OFF_LADDER[rng.integers(0, len(M.OFF_LADDER), int((cols < 0.15).sum()))]
            f["old_color"][yy, (cols >= 0.15) & (cols < 0.2), 0] = np.nan
            f["old_color"][yy, (cols >= 0.2) & (cols < 0.23), 1] = np.inf
            far = (cols >= 0.23) & (cols < 0.28) & (f["old_nd"][yy, :, 3] > 0)
            f["old_nd"][yy, far, 3] *= np.float32(1.5)
    p = (0.5, 0.98, 1e-2)
    want = oracle_temporal(O, f, p)
    rows_needed = H.halo_rows_for_motion(Camera(*f["old"]), Camera(*f["new"]), w, h, near=0.25, band_rows=band)
    halo_rows = max(1, min(rows_needed, band))
    rt = hip()
    ctxs = [new_context(H, scenes, noise, w, h, rank=r, nranks=nranks, band_rows=band) for r in range(nranks)]
    bufs = []
    try:
        rows = [c.local_rows() for c in ctxs]
        for c, rr in zip(ctxs, rows):
            c.set_option(OPT_HALO_ROWS, halo_rows)
            inject(rt, c, f, p, rows=rr, current=False)
        for c in ctxs:
            pb, nb = C.c_void_p(), C.c_void_p()
            nbytes = c.halo_bytes()
            assert nbytes > 0 and rt.hipMalloc(C.byref(pb), nbytes) == 0 and rt.hipMalloc(C.byref(nb), nbytes) == 0
            bufs.append((pb, nb))
            c.halo_export(pb.value, nb.value)
        got = np.zeros_like(want)
        for r, (c, rr) in enumerate(zip(ctxs, rows)):
            c.halo_import(bufs[(r - 1) % nranks][1].value, bufs[(r + 1) % nranks][0].value)
            inject(rt, c, f, p, rows=rr, history=False)
            c.render_stage(TEMPORAL)
            got[rr] = c.read(ACCUM_COLOR)
        for c in ctxs:
            c.sync()
    finally:
        for c in ctxs:
            c.close()
        for pb, nb in bufs:
            rt.hipFree(pb)
            rt.hipFree(nb)
    assert_bits_equal(got, want, f"{nranks} ranks, {band}-row bands, {motion}, halo rows {halo_rows}")
    # coverage: accepted pixels whose history rows (those of non-zero weight) belong to another rank
    ref = model(f, p)
    owner = np.empty(h, np.int64)
    for r, rr in enumerate(rows):
        owner[rr] = r
    ys, xs = np.nonzero(ref["accepted"])
    y0 = np.floor(ref["fy"][ys, xs]).astype(np.int64)
    ay = ref["ay"][ys, xs]
    ra, rb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    foreign = ((ay != 1) & (owner[ra] != owner[ys])) | ((ay != 0) & (owner[rb] != owner[ys]))
    assert foreign.sum() >= 10, (int(foreign.sum()), halo_rows)
    edge_rows = np.isin(np.arange(h) % band, (band - 2, band - 1, 0, 1))
    assert (np.isnan(want[..., :3]).any(-1) & edge_rows[:, None]).any()   # the salted rows reach the output
    assert not M.disagreement(got, ref).any()
