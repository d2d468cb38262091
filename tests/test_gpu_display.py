"""GPU: the displayed frame (include/vxrt.h: VXRT_DISPLAY_BGRA8_SRGB / VXRT_DISPLAY_RGBA8_SRGB) — VXRT_DENOISED encoded to 8-bit sRGB on
the device by the library's exact rule, read back at 4 bytes per pixel through every path: vxrt_read, vxrt_read_async, vxrt_device_image,
and a rank's band set.  The oracle is the rule in binary64 (test_display_cpu.display_oracle)."""
import ctypes as C

import numpy as np
import pytest

from test_display_cpu import BGRA, RGBA, display_oracle, threshold_windows

pytestmark = pytest.mark.gpu


def hip():
    lib = C.CDLL("libamdhip64.so")
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    lib.hipMemcpy.restype = C.c_int
    return lib


HOST_TO_DEVICE, DEVICE_TO_HOST = 1, 2


def assert_bytes_equal(got, want, what):
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape, got.dtype)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} bytes differ; first at {tuple(bad[0])}: {got[tuple(bad[0])]} vs {want[tuple(bad[0])]}"


def special_values():
    f = np.float32
    bits = np.array([0x7fc00000, 0xffc00000, 0x7fc00001, 0x7fa00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffffffff,   # quiet / signalling NaNs, payloads
                     0x00000001, 0x00000010, 0x007fffff, 0x80000001, 0x807fffff, 0x00800000], np.uint32).view(np.float32)  # denormals, smallest normal
    b = f(0.0031308)
    vals = [0.0, -0.0, np.inf, -np.inf, np.finfo(f).max, -np.finfo(f).max, 1.0, np.nextafter(f(1), f(0)), np.nextafter(f(1), f(2)), -1.0, 0.5,
            b, np.nextafter(b, f(0)), np.nextafter(b, f(1)), np.nextafter(np.nextafter(b, f(1)), f(1)), 2.0, 1e-30]
    return np.concatenate([bits, np.array(vals, np.float32)])


def probe_inputs(H):
    t = H.display_thresholds()
    rng = np.random.default_rng(20261015)
    parts = [threshold_windows(t, 64), special_values(), rng.integers(0, 2 ** 32, 4 * 1024 * 1024, dtype=np.uint64).astype(np.uint32).view(np.float32),
             np.arange(0, 0x3f800001, 256, dtype=np.uint32).view(np.float32), t]
    return np.concatenate(parts)


def test_probe_equals_the_rule_on_every_tested_input(H):
    """±64 ULP around every threshold, the specials, 4 M random bit patterns, every 256th bit pattern of [0, 1]: each value through every
    channel position (colour and alpha), both byte orders.  The pixel count is not a multiple of 4 (the kernel's tail)."""
    x = probe_inputs(H)
    x = np.concatenate([x, np.zeros((-len(x)) % 4, np.float32)])            # whole pixels ...
    if (len(x) // 4) % 4 == 0:
        x = np.concatenate([x, np.full(4, 0.5, np.float32)])                 # ... and a tail
    assert (len(x) // 4) % 4 != 0
    for shift in range(4):
        px = np.roll(x, shift).reshape(-1, 4)
        for fmt in (BGRA, RGBA):
            assert_bytes_equal(H.display_encode(px, fmt), display_oracle(px, fmt), f"probe shift {shift} format {fmt}")
    with pytest.raises(H.VxrtError):
        H.display_encode(np.zeros((4, 4), np.float32), 4)
    for n in (1, 2, 3, 5, 7):          # tails alone
        px = np.tile(np.array([[0.5, np.nan, 1.0, 0.25]], np.float32), (n, 1))
        assert_bytes_equal(H.display_encode(px, BGRA), display_oracle(px, BGRA), f"{n} pixels")


def _ctx(scenes, noise, scene="castle", w=200, h=120, bounces=3, camera="close", **kw):
    from gpu_voxel_raytracer_amd import Camera, Context
    pos, mrgb, size = scenes.load_scene(scene)
    ctx = Context(w, h, max_bounces=bounces, noise=noise, **kw)
    ctx.recreate_octree(pos, mrgb)
    ctx.camera = Camera(*(scenes.close_camera(size) if camera == "close" else scenes.bench_camera(size)))
    ctx.denoise_uniforms.radius = 2
    return ctx


@pytest.mark.parametrize("scene,w,h,bounces,camera", [("castle", 200, 120, 3, "close"), ("menger", 640, 360, 4, "bench")])
def test_rendered_frames_equal_the_oracle_of_the_denoised_image(H, scenes, noise, scene, w, h, bounces, camera):
    from gpu_voxel_raytracer_amd import ALL, DENOISED, DISPLAY_BGRA8_SRGB, DISPLAY_RGBA8_SRGB
    with _ctx(scenes, noise, scene, w, h, bounces, camera) as ctx:
        for frame in range(3):
            ctx.render(ALL)
            den = ctx.read(DENOISED)
            bgra, rgba = ctx.read(DISPLAY_BGRA8_SRGB), ctx.read(DISPLAY_RGBA8_SRGB)
            assert bgra.shape == (h, w, 4) and bgra.dtype == np.uint8
            assert_bytes_equal(bgra, display_oracle(den, BGRA), f"{scene} frame {frame + 1} BGRA")
            assert_bytes_equal(rgba, display_oracle(den, RGBA), f"{scene} frame {frame + 1} RGBA")
            assert_bytes_equal(bgra, rgba[..., [2, 1, 0, 3]], "BGRA is RGBA with R and B swapped")
            assert np.all(bgra[..., 3] == 255)
            assert len(np.unique(rgba[..., :3])) > 16                # a real picture, not a flat one


def test_injected_values_reach_every_read_path_exactly(H, scenes, noise):
    """Crafted floats written into the DENOISED image itself (NaN, inf, negative, threshold neighbours; 45 x 23 pixels, not a multiple of
    4) come out of vxrt_read, vxrt_read_async and vxrt_device_image as the rule says."""
    from gpu_voxel_raytracer_amd import DENOISED, DISPLAY_BGRA8_SRGB, DISPLAY_RGBA8_SRGB, Context
    rt = hip()
    w, h = 45, 23
    pool = np.concatenate([special_values(), threshold_windows(H.display_thresholds(), 2)])
    img = np.resize(np.random.default_rng(5).permutation(pool), (h, w, 4)).astype(np.float32)
    with Context(w, h, noise=noise) as ctx:
        ptr, nbytes = ctx.device_image(DENOISED)
        assert nbytes == img.nbytes
        ctx.sync()
        assert rt.hipMemcpy(ptr, img.ctypes.data, nbytes, HOST_TO_DEVICE) == 0
        got = ctx.read(DENOISED)
        assert np.array_equal(got.view(np.uint32), img.view(np.uint32))
        for fmt, which in ((BGRA, DISPLAY_BGRA8_SRGB), (RGBA, DISPLAY_RGBA8_SRGB)):
            want = display_oracle(img, fmt)
            assert_bytes_equal(ctx.read(which), want, f"vxrt_read {which}")
            buf = ctx.pinned_display()
            ctx.read_async(which, buf, 1)
            ctx.read_wait(1)
            assert_bytes_equal(buf.array, want, f"vxrt_read_async {which}")
            buf.close()
            dptr, dbytes = ctx.device_image(which)
            assert dbytes == w * h * 4
            ctx.sync()
            dev = np.zeros((h, w, 4), np.uint8)
            assert rt.hipMemcpy(dev.ctypes.data, dptr, dbytes, DEVICE_TO_HOST) == 0
            assert_bytes_equal(dev, want, f"vxrt_device_image {which}")


@pytest.mark.parametrize("inflight,batch", [(1, 1), (2, 4)])
def test_a_display_transfer_carries_the_frame_it_was_asked_for(H, scenes, noise, inflight, batch):
    """Frames keep being rendered while earlier frames travel at 4 bytes per pixel: every transfer holds ITS frame (the encode runs on the
    context's stream before later stages may overwrite the denoised image), slots alternate, nothing is waited for until the end."""
    from gpu_voxel_raytracer_amd import ALL, DISPLAY_BGRA8_SRGB, DISPLAY_RGBA8_SRGB
    with _ctx(scenes, noise, frames_in_flight=inflight, frames_per_launch=batch) as ref:
        want = []
        for f in range(4):
            ref.render(ALL)
            want.append((ref.read(DISPLAY_BGRA8_SRGB), ref.read(DISPLAY_RGBA8_SRGB)))
    assert not np.array_equal(want[0][0], want[3][0])                 # the frames differ: a stale transfer would show
    with _ctx(scenes, noise, frames_in_flight=inflight, frames_per_launch=batch) as ctx:
        bufs = [ctx.pinned_display(), ctx.pinned_display()]
        got = []
        for f in range(4):
            ctx.render(ALL)
            if f >= 2:
                ctx.read_wait(f & 1)
                got.append(bufs[f & 1].array.copy())
            ctx.read_async(DISPLAY_BGRA8_SRGB if f % 3 else DISPLAY_RGBA8_SRGB, bufs[f & 1], f & 1)
        for f in (2, 3):
            ctx.read_wait(f & 1)
            got.append(bufs[f & 1].array.copy())
        for f in range(4):
            assert_bytes_equal(got[f], want[f][0 if f % 3 else 1], f"display frame {f + 1}")
        for b in bufs:
            b.close()


def test_a_rank_s_display_rows_interleave_into_the_single_context_s(H, scenes, noise):
    from gpu_voxel_raytracer_amd import ALL, DISPLAY_BGRA8_SRGB, DISPLAY_RGBA8_SRGB
    w, h = 200, 120
    with _ctx(scenes, noise, w=w, h=h) as single:
        single.denoise_uniforms.radius = 0
        ranks = [_ctx(scenes, noise, w=w, h=h, rank=r, nranks=2, band_rows=16) for r in range(2)]
        try:
            for c in ranks:
                c.denoise_uniforms.radius = 0
            for frame in range(2):
                single.render(ALL)
                for c in ranks:
                    c.render(ALL)
                for which in (DISPLAY_BGRA8_SRGB, DISPLAY_RGBA8_SRGB):
                    want = single.read(which)
                    got = np.zeros_like(want)
                    for c in ranks:
                        rows = c.local_rows()
                        assert 0 < len(rows) < h
                        part = c.read(which)
                        buf = c.pinned_display()
                        c.read_async(which, buf, frame & 1)
                        c.read_wait(frame & 1)
                        assert_bytes_equal(buf.array, part, "async band set")
                        buf.close()
                        got[rows] = part
                    assert_bytes_equal(got, want, f"frame {frame + 1} image {which}")
        finally:
            for c in ranks:
                c.close()


def test_device_display_image_follows_the_frame_and_resize(H, scenes, noise):
    from gpu_voxel_raytracer_amd import ALL, DISPLAY_BGRA8_SRGB
    rt = hip()
    with _ctx(scenes, noise) as ctx:
        for w, h in ((200, 120), (320, 176)):
            if w != 200:
                ctx.resize(w, h)
            ctx.render(ALL)
            ptr, nbytes = ctx.device_image(DISPLAY_BGRA8_SRGB)
            assert ptr and nbytes == w * h * 4
            ctx.sync()
            dev = np.zeros((h, w, 4), np.uint8)
            assert rt.hipMemcpy(dev.ctypes.data, ptr, nbytes, DEVICE_TO_HOST) == 0
            assert_bytes_equal(dev, ctx.read(DISPLAY_BGRA8_SRGB), f"device image {w}x{h}")


def test_bad_arguments_are_refused(H, scenes, noise):
    from gpu_voxel_raytracer_amd import ALL, DISPLAY_BGRA8_SRGB, DISPLAY_RGBA8_SRGB
    with _ctx(scenes, noise) as ctx:
        ctx.render(ALL)
        L, hd = ctx._L, ctx._h
        f32 = np.zeros((120, 200, 4), np.float32)
        u8 = np.zeros((120, 200, 4), np.uint8)
        p32, p8 = f32.ctypes.data_as(C.c_void_p), u8.ctypes.data_as(C.c_void_p)
        for which in (DISPLAY_BGRA8_SRGB, DISPLAY_RGBA8_SRGB):
            assert L.vxrt_read(hd, C.c_int(which), p32, C.c_size_t(f32.nbytes)) == H.E_INVALID                          # the rgba32f size
            assert L.vxrt_read_async(hd, C.c_int(which), p32, C.c_size_t(f32.nbytes), C.c_uint32(0)) == H.E_INVALID
            assert L.vxrt_read(hd, C.c_int(which), None, C.c_size_t(u8.nbytes)) == H.E_INVALID
            assert L.vxrt_read_async(hd, C.c_int(which), None, C.c_size_t(u8.nbytes), C.c_uint32(0)) == H.E_INVALID
            assert L.vxrt_read_async(hd, C.c_int(which), p8, C.c_size_t(u8.nbytes), C.c_uint32(2)) == H.E_INVALID      # slot
            assert L.vxrt_read(hd, C.c_int(which), p8, C.c_size_t(u8.nbytes)) == 0
        for bad in (7, 9):
            assert L.vxrt_read(hd, C.c_int(bad), p8, C.c_size_t(u8.nbytes)) == H.E_INVALID
            assert L.vxrt_read_async(hd, C.c_int(bad), p8, C.c_size_t(u8.nbytes), C.c_uint32(0)) == H.E_INVALID
            ptr, n = C.c_void_p(), C.c_size_t(0)
            assert L.vxrt_device_image(hd, C.c_int(bad), C.byref(ptr), C.byref(n)) == H.E_INVALID
        assert L.vxrt_read_wait(hd, C.c_uint32(0)) == 0


def test_frame_loop_gpu_and_cpu_encodes_write_the_same_pngs(tmp_path):
    from gpu_voxel_raytracer_amd import frame_loop
    outs = {}
    for enc in ("cpu", "gpu"):
        base = str(tmp_path / enc / "frame")
        frame_loop.run("menger:4", 160, 90, frames=3, bounces=3, radius=2, out=base, dump_every=1, encode=enc)
        outs[enc] = [open(f"{base}{suffix}.png", "rb").read() for suffix in ("_0001", "_0002", "_0003", "")]
    assert outs["cpu"] == outs["gpu"]
