"""GPU: denoise.comp (shaders/denoise.comp:24-93) on SYNTHETIC G-buffers written straight into the context's images, so that the
inputs the traced scenes rarely produce are all there: colours and depths that are 0 / inf / NaN, normals that are not axis unit
vectors, every material id, window edges of the frame.  The fast kernel (two outputs per lane, one code compare instead of the normal
and material terms — csrc/post.hip: denoise_pair_kernel) and the generic kernel (the full formula per tap) must both equal the
oracle bit for bit in exact mode; the tolerant mode stays within BASELINE's RMSE bar."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu


def hip():
    lib = C.CDLL("libamdhip64.so")
    lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return lib


def synthetic_gbuffer(w, h, seed, exotic, radius=1):
    """colour (rgb, blending), normal/depth, albedo/node: float32[h, w, 4] each."""
    rng = np.random.default_rng(seed)
    f32 = np.float32
    color = rng.random((h, w, 4)).astype(f32) * f32(3.0)
    # surfaces: blocks of equal normal / material / similar depth, so that most taps carry weight
    by, bx = np.mgrid[0:h, 0:w]
    patch = (by // 9) * 7 + (bx // 11)
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0]], f32)
    nd = np.zeros((h, w, 4), f32)
    nd[..., :3] = axes[patch % 7]
    nd[..., 3] = (f32(4.0) + (patch % 5).astype(f32) + rng.random((h, w)).astype(f32) * f32(0.05))
    node = (np.uint32(0x80000000) | ((patch % 3).astype(np.uint32) << np.uint32(24)) | rng.integers(0, 1 << 24, (h, w)).astype(np.uint32))
    sky = rng.random((h, w)) < 0.15                                     # misses: normal 2^30, depth -1, node 0xffffff
    nd[sky, :3] = f32(2.0 ** 30)
    nd[sky, 3] = f32(-1.0)
    node[sky] = np.uint32(0xffffff)
    alb = rng.random((h, w, 4)).astype(f32)
    alb[..., 3] = node.view(f32)
    if exotic:
        thin = 9.0 / (2 * radius + 1) ** 2                              # a non-finite pixel poisons its whole window: keep most of the frame finite
        pick = lambda p: rng.random((h, w)) < p * thin                  # noqa: E731
        color[pick(0.004), 0] = np.inf
        color[pick(0.004), 1] = np.nan
        color[pick(0.003), 2] = -np.inf
        nd[pick(0.004), 3] = 0.0                                        # log 0 = -inf
        nd[pick(0.004), 3] = np.nan
        nd[pick(0.003), 3] = np.inf
        odd = pick(0.01)
        nd[odd, :3] = np.array([0.6, 0.8, 0.0], f32)                    # not an axis vector
        nd[pick(0.003), 0] = np.nan
        nd[pick(0.003), 1] = f32(-0.0)
    return color, nd, alb


def run_denoise(H, scenes, noise, color, nd, alb, radius, mode, sigma_range=1.5, sigma_distance=2.0, albedo_factor=1.0):
    from gpu_voxel_raytracer_amd import DENOISE, DENOISED, NORMAL_DEPTH, SAMPLED_COLOR, ALBEDO_NODE, TRACE, Camera, Context
    h, w = color.shape[:2]
    pos, mrgb, size = scenes.load_scene("8x8x8")
    cam = scenes.bench_camera(size)
    rt = hip()
    with Context(w, h, max_bounces=1, noise=noise) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = Camera(*cam)
        ctx.render(TRACE)                     # a frame slot exists and is current
        ctx.sync()
        for which, img in ((SAMPLED_COLOR, color), (NORMAL_DEPTH, nd), (ALBEDO_NODE, alb)):
            ptr, nbytes = ctx.device_image(which)
            assert nbytes == img.nbytes
            assert rt.hipMemcpy(C.c_void_p(ptr), img.ctypes.data_as(C.c_void_p), nbytes, 1) == 0
        ctx.denoise_uniforms.radius = radius
        ctx.denoise_uniforms.sigma_range = sigma_range
        ctx.denoise_uniforms.sigma_distance = sigma_distance
        ctx.denoise_uniforms.albedo_factor = albedo_factor
        ctx.set_option(H.OPT_DENOISE_MODE, mode)
        ctx.update_bindings()
        ctx.render_stage(DENOISE)
        return ctx.read(DENOISED), cam


def oracle_denoise(O, color, nd, alb, cam, radius, sigma_range=1.5, sigma_distance=2.0, albedo_factor=1.0):
    h, w = color.shape[:2]
    u = O.Uniforms.default()
    u.set_camera(cam[0], O.camera_axis_scaled(cam[0], cam[1], cam[2], w, h))
    du = O.Denoise.default()
    du.radius, du.sigma_range, du.sigma_distance, du.albedo_factor = radius, sigma_range, sigma_distance, albedo_factor
    return O.denoise(color, nd, alb, u.camera16(), du)


@pytest.mark.parametrize("w,h,radius,exotic", [(70, 50, 1, True), (97, 33, 2, True), (64, 64, 5, True), (131, 70, 8, True), (40, 23, 8, False),
                                             (33, 17, 3, True)])
def test_exact_denoise_equals_the_oracle_on_synthetic_gbuffers(O, H, scenes, noise, w, h, radius, exotic):
    color, nd, alb = synthetic_gbuffer(w, h, seed=w * 1000 + h + radius, exotic=exotic, radius=radius)
    fast, cam = run_denoise(H, scenes, noise, color, nd, alb, radius, mode=0)
    generic, _ = run_denoise(H, scenes, noise, color, nd, alb, radius, mode=2)
    want = oracle_denoise(O, color, nd, alb, cam, radius)
    assert np.isfinite(want[..., :3]).mean() > 0.4 and (not exotic or np.isnan(want[..., :3]).any())
    assert_bits_equal(generic, want, f"generic kernel, radius {radius}")
    assert_bits_equal(fast, want, f"fast kernel, radius {radius}")


@pytest.mark.parametrize("sigma_range,sigma_distance,albedo_factor", [(0.1, 0.5, 0.0), (5.0, 3.0, 0.5), (7.0, 2.0, 1.0), (8.0, 2.0, 1.0), (40.0, 1.0, 0.3)])
def test_denoise_parameter_range(O, H, scenes, noise, sigma_range, sigma_distance, albedo_factor):
    """sigma_range up to 7 (the GUI offers 0.1 .. 5, src/context.rs:1798): the fast kernel's premise holds (1e4 / (2 sigma^2) > 100); beyond it
    a tap of another material can carry weight and launch_denoise takes the generic kernel — bit-exact either way."""
    color, nd, alb = synthetic_gbuffer(90, 60, seed=int(sigma_range * 10), exotic=True, radius=4)
    got, cam = run_denoise(H, scenes, noise, color, nd, alb, 4, 0, sigma_range, sigma_distance, albedo_factor)
    want = oracle_denoise(O, color, nd, alb, cam, 4, sigma_range, sigma_distance, albedo_factor)
    assert_bits_equal(got, want, f"sigma_range {sigma_range}")


@pytest.mark.parametrize("radius,mode", [(2, 1), (8, 1), (8, 3)])
def test_tolerant_denoise_on_synthetic_gbuffers(O, H, scenes, noise, radius, mode):
    color, nd, alb = synthetic_gbuffer(128, 96, seed=radius, exotic=False)
    got, cam = run_denoise(H, scenes, noise, color, nd, alb, radius, mode)
    want = oracle_denoise(O, color, nd, alb, cam, radius)
    err = got[..., :3].astype(np.float64) - want[..., :3]
    assert np.sqrt(np.mean(err ** 2)) <= 1e-5 and np.abs(err).max() <= 1e-4         # BASELINE's bar is RMSE <= 1e-3


@pytest.mark.parametrize("nranks,band,radius,split", [(2, 16, 3, False), (3, 32, 8, True), (2, 48, 8, True)])
def test_exotic_pixels_across_band_edges(O, H, scenes, noise, nranks, band, radius, split):
    """The same synthetic G-buffer dealt to N contexts in row bands: non-finite colours, zero / NaN depths and odd normals sit in the
    HALO rows too, where the fast kernel's literal path fetches its operands from the halo store instead of the rank's own images.
    Stitched output equals the oracle's, with the denoise stage whole and split around the exchange."""
    from gpu_voxel_raytracer_amd import (DENOISE, DENOISE_EDGE, DENOISE_INTERIOR, DENOISED, NORMAL_DEPTH, SAMPLED_COLOR, ALBEDO_NODE, TRACE,
                                         Camera, Context)
    w, h = 96, 200
    color, nd, alb = synthetic_gbuffer(w, h, seed=nranks * 100 + band + radius, exotic=True, radius=radius)
    pos, mrgb, size = scenes.load_scene("8x8x8")
    cam = scenes.bench_camera(size)
    want = oracle_denoise(O, color, nd, alb, cam, radius)
    rt = hip()
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    ctxs = [Context(w, h, max_bounces=1, noise=noise, rank=r, nranks=nranks, band_rows=band) for r in range(nranks)]
    try:
        rows = []
        for c in ctxs:
            c.recreate_octree(pos, mrgb)
            c.camera = Camera(*cam)
            c.render(TRACE)
            c.sync()
            rr = c.local_rows()
            rows.append(rr)
            for which, img in ((SAMPLED_COLOR, color), (NORMAL_DEPTH, nd), (ALBEDO_NODE, alb)):
                ptr, nbytes = c.device_image(which)
                mine = np.ascontiguousarray(img[rr])
                assert nbytes == mine.nbytes
                assert rt.hipMemcpy(C.c_void_p(ptr), mine.ctypes.data_as(C.c_void_p), nbytes, 1) == 0
            c.denoise_uniforms.radius = radius
            c.update_bindings()
        bufs = {}
        for r, c in enumerate(ctxs):
            p, n = C.c_void_p(), C.c_void_p()
            nbytes = c.halo_bytes()
            assert rt.hipMalloc(C.byref(p), nbytes) == 0 and rt.hipMalloc(C.byref(n), nbytes) == 0
            c.halo_export(p.value, n.value)
            bufs[r] = (p, n)
            if split:
                c.render_stage(DENOISE_INTERIOR)
        got = np.zeros_like(want)
        for r, c in enumerate(ctxs):
            c.halo_import(bufs[(r - 1) % nranks][1].value, bufs[(r + 1) % nranks][0].value)
            c.render_stage(DENOISE_EDGE if split else DENOISE)
            got[rows[r]] = c.read(DENOISED)
        assert np.isnan(want[..., :3]).any() and np.isfinite(want[..., :3]).mean() > 0.4
        assert_bits_equal(got, want, f"{nranks} ranks, {band}-row bands, radius {radius}")
    finally:
        for c in ctxs:
            c.close()


# ---- every compiled variant against the oracle ------------------------------------------------------------------------------------
# launch_denoise (csrc/post.hip) picks one of: the pass-through kernel (radius 0), denoise_pair_kernel<tolerant, r> for r = 1 .. 8
# (VXRT_PAIR), denoise_generic_kernel<tolerant>.  Inside a pair kernel each 32x16 output tile takes the LEAN loop (no exotic pixel in
# its apron: pair_window<.., true, r>, unrolled) or the CAREFUL one (pair_window<.., false, 0> and literal_window for exotic centres).
# The G-buffers below put exotic pixels only where a test wants them, so that every case holds blocks of both kinds.

PAIR_RADII = tuple(range(1, 9))          # the radii of VXRT_PAIR(..) and vxrt_set_denoise's bound (tests/test_denoise_variants_cpu.py)
SWEEP_RADII = (0,) + PAIR_RADII
MODES = (0, 1, 2, 3)                     # VXRT_OPT_DENOISE_MODE: 1 = tolerant, + 2 = the generic kernel
PAIR_TILE_W, PAIR_TILE_H = 32, 16        # denoise_pair_kernel's output tile

_F32 = np.float32
_PLAIN_NORMALS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1],
                           [-0.0, -0.0, 1], [0, -1, -0.0], [-0.0, 0, 0]], _F32)
_PLAIN_NORMAL_BITS = np.array([0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x4e800000], np.uint32)   # +-0, +-1, 2^30


def _poison_r(c, n):
    c[0] = np.inf


def _poison_g(c, n):
    c[1] = np.nan


def _poison_b(c, n):
    c[2] = -np.inf


def _depth_zero(c, n):
    n[3] = -0.0                          # log 0 = -inf


def _depth_nan(c, n):
    n[3] = np.nan


def _depth_inf(c, n):
    n[3] = np.inf


def _normal_oblique(c, n):
    n[:3] = (0.6, 0.8, 0.0)              # finite, but not an axis vector


def _normal_nan(c, n):
    n[0] = np.nan


def _normal_half(c, n):
    n[:3] = (0.0, 0.0, 0.5)


def _normal_neg_sky(c, n):
    n[:3] = -(2.0 ** 30)                 # -2^30 is not the sky's code


EXOTIC_KINDS = (_poison_r, _normal_oblique, _depth_zero, _poison_g, _normal_nan, _depth_nan, _poison_b, _normal_half, _depth_inf,
                _normal_neg_sky)
FINITE_EXOTIC_KINDS = (_normal_oblique, _normal_half, _normal_neg_sky)   # exotic, but they poison no window


def planned_gbuffer(w, h, seed, exotic_at=(), kinds=EXOTIC_KINDS):
    """colour, normal/depth, albedo/node (float32[h, w, 4] each) whose only exotic pixels are those of `exotic_at` ((y, x) pairs; the
    k-th gets kinds[k % len(kinds)]).  Everywhere else every plain code a traced frame holds: the sky (2^30 normal, depth -1), the six
    axes, normals with +-0 components, four materials, patches of equal code with close depths so that most taps carry weight."""
    rng = np.random.default_rng(seed)
    color = rng.random((h, w, 4)).astype(_F32) * _F32(3.0)
    by, bx = np.mgrid[0:h, 0:w]
    patch = (by // 5) * 7 + (bx // 6)
    nd = np.zeros((h, w, 4), _F32)
    nd[..., :3] = _PLAIN_NORMALS[patch % len(_PLAIN_NORMALS)]
    nd[..., 3] = _F32(4.0) + (patch % 5).astype(_F32) + rng.random((h, w)).astype(_F32) * _F32(0.05)
    node = np.uint32(0x80000000) | ((patch % 4).astype(np.uint32) << np.uint32(24)) | rng.integers(0, 1 << 24, (h, w)).astype(np.uint32)
    sky = rng.random((h, w)) < 0.15
    nd[sky, :3] = _F32(2.0 ** 30)
    nd[sky, 3] = _F32(-1.0)
    node[sky] = np.uint32(0xffffff)
    alb = rng.random((h, w, 4)).astype(_F32)
    alb[..., 3] = node.view(_F32)
    for k, (y, x) in enumerate(exotic_at):
        kinds[k % len(kinds)](color[y, x], nd[y, x])
    return color, nd, alb


def exotic_pixels(color, nd):
    """The pair kernel's 'exotic' pixels: a colour or log|depth| that is not finite, or a normal component other than +-0, +-1, 2^30."""
    with np.errstate(divide="ignore", invalid="ignore"):
        logd_finite = np.isfinite(np.log(np.abs(nd[..., 3].astype(np.float64))))
    odd_normal = ~np.isin(np.ascontiguousarray(nd[..., :3]).view(np.uint32), _PLAIN_NORMAL_BITS).all(axis=-1)
    return ~np.isfinite(color[..., :3]).all(axis=-1) | ~logd_finite | odd_normal


def careful_blocks(exotic, radius, rows=None):
    """bool[tile rows, tile columns]: which blocks of denoise_pair_kernel take the careful loop.  A block makes the 32x16 output tile of
    local rows 16 t .. 16 t + 15 and stages the frame rows frame_row(16 t) - r .. + 15 + r, columns 32 c - r .. 32 c + 31 + r; it is
    careful when any of them is exotic.  rows: the frame rows of a rank's local rows (banded); None: the whole frame."""
    h, w = exotic.shape
    rows = np.arange(h) if rows is None else np.asarray(rows)
    careful = np.zeros(((len(rows) + PAIR_TILE_H - 1) // PAIR_TILE_H, (w + PAIR_TILE_W - 1) // PAIR_TILE_W), bool)
    for t in range(careful.shape[0]):
        y0 = int(rows[t * PAIR_TILE_H])
        for c in range(careful.shape[1]):
            x0 = c * PAIR_TILE_W
            careful[t, c] = exotic[max(0, y0 - radius):y0 + PAIR_TILE_H + radius, max(0, x0 - radius):x0 + PAIR_TILE_W + radius].any()
    return careful


def assert_both_paths(exotic, radius, what, rows=None):
    careful = careful_blocks(exotic, radius, rows)
    if careful.size > 1:
        assert careful.any() and not careful.all(), f"{what}: blocks should be both lean and careful: {careful.astype(int).tolist()}"


def assert_tolerant_close(got, want, what, exotic=None):
    """Tolerant mode: the same NaN / +inf / -inf pixels per channel as the oracle, within the RMSE / max bar where both are finite;
    with `exotic` (the fast kernel), those centres are made by literal_window and equal the oracle bit for bit."""
    g, wv = got[..., :3], want[..., :3]
    for name, test in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        for ch in range(3):
            diff = test(g[..., ch]) != test(wv[..., ch])
            assert not diff.any(), f"{what}: {name} mask of channel {ch} differs at {int(diff.sum())} pixels, first {tuple(np.argwhere(diff)[0])}"
    both = np.isfinite(g) & np.isfinite(wv)
    err = g[both].astype(np.float64) - wv[both]
    if err.size:
        rmse, worst = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
        assert rmse <= 1e-5 and worst <= 1e-4, f"{what}: RMSE {rmse:.3e}, max abs {worst:.3e}"
    assert (got[..., 3] == 1).all(), what
    if exotic is not None and exotic.any():
        assert_bits_equal(got[exotic], want[exotic], f"{what}: exotic centres (literal_window)")


# (w, h) -> the exotic pixels: frame corners and edges, and a few inside chosen tiles.  Both frames of several tiles keep lean blocks
# at every radius; the frames smaller than a window are one or two blocks.
SWEEP_FRAMES = {
    (97, 49): [(0, 0), (0, 96), (48, 0), (48, 96), (20, 0), (0, 80),           # corners, edges
               (38, 75), (39, 76), (40, 75), (45, 90), (44, 72)],             # inside tile (2, 2)
    (64, 32): [(0, 0), (31, 63), (5, 9), (6, 9), (10, 20)],                    # two corners, inside tile (0, 0)
    (1, 1): [],
    (3, 2): [(0, 0)],
    (2, 19): [(0, 1), (1, 0)],
    (40, 1): [(0, 0), (0, 5)],
}


class SyntheticFrame:
    """One Context holding a planned G-buffer; denoise() runs the stage again with other uniforms / mode (update_bindings between)."""

    def __init__(self, H, scenes, noise, w, h, exotic_at):
        from gpu_voxel_raytracer_amd import ALBEDO_NODE, NORMAL_DEPTH, SAMPLED_COLOR, TRACE, Camera, Context
        kinds = EXOTIC_KINDS if w * h > 64 else FINITE_EXOTIC_KINDS   # a tiny frame keeps finite outputs to compare
        self.color, self.nd, self.alb = planned_gbuffer(w, h, seed=w * 1000 + h, exotic_at=exotic_at, kinds=kinds)
        self.exotic = exotic_pixels(self.color, self.nd)
        assert self.exotic.sum() == len(set(exotic_at))
        self.H = H
        pos, mrgb, size = scenes.load_scene("8x8x8")
        self.cam = scenes.bench_camera(size)
        self.ctx = Context(w, h, max_bounces=1, noise=noise)
        self.ctx.recreate_octree(pos, mrgb)
        self.ctx.camera = Camera(*self.cam)
        self.ctx.render(TRACE)
        self.ctx.sync()
        rt = hip()
        for which, img in ((SAMPLED_COLOR, self.color), (NORMAL_DEPTH, self.nd), (ALBEDO_NODE, self.alb)):
            ptr, nbytes = self.ctx.device_image(which)
            assert nbytes == img.nbytes
            assert rt.hipMemcpy(C.c_void_p(ptr), img.ctypes.data_as(C.c_void_p), nbytes, 1) == 0

    def denoise(self, radius, mode, sigma_range=1.5, sigma_distance=2.0, albedo_factor=1.0):
        from gpu_voxel_raytracer_amd import DENOISE, DENOISED
        u = self.ctx.denoise_uniforms
        u.radius, u.sigma_range, u.sigma_distance, u.albedo_factor = radius, sigma_range, sigma_distance, albedo_factor
        self.ctx.set_option(self.H.OPT_DENOISE_MODE, mode)
        self.ctx.update_bindings()
        self.ctx.render_stage(DENOISE)
        return self.ctx.read(DENOISED)

    def oracle(self, O, radius, **uniforms):
        return oracle_denoise(O, self.color, self.nd, self.alb, self.cam, radius, **uniforms)


@pytest.fixture(scope="module")
def frames(H, scenes, noise):
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = SyntheticFrame(H, scenes, noise, w, h, SWEEP_FRAMES[(w, h)])
        return made[(w, h)]
    yield get
    for f in made.values():
        f.ctx.close()


@pytest.mark.parametrize("radius", SWEEP_RADII, ids=[f"r{r}" for r in SWEEP_RADII])
@pytest.mark.parametrize("w,h", list(SWEEP_FRAMES), ids=[f"{w}x{h}" for w, h in SWEEP_FRAMES])
def test_every_denoise_variant_equals_the_oracle(O, frames, w, h, radius):
    """Radius 0 .. 8 x VXRT_OPT_DENOISE_MODE 0 .. 3 on one frame: exact modes and radius 0 bit-equal to the oracle; tolerant modes
    with the oracle's non-finite pixels, close elsewhere, and (fast kernel) its exotic centres exact."""
    f = frames(w, h)
    want = f.oracle(O, radius)
    if radius > 0:
        assert_both_paths(f.exotic, radius, f"{w}x{h}, radius {radius}")
    if w * h > 64:
        assert np.isfinite(want[..., :3]).mean() > 0.3 and (not f.exotic.any() or np.isnan(want[..., :3]).any())
    else:
        assert np.isfinite(want[..., :3]).all()
    for mode in MODES:
        got = f.denoise(radius, mode)
        what = f"{w}x{h}, radius {radius}, mode {mode}"
        if radius == 0 or mode in (0, 2):
            assert_bits_equal(got, want, what)
        else:
            assert_tolerant_close(got, want, what, exotic=f.exotic if mode == 1 else None)


def fast_sigma_range_edge():
    """(the largest binary32 sigma_range for which launch_denoise takes the fast kernel, the next value up), found with the host's
    binary32 arithmetic: sigma_range_2 = 2 (s s), fast while 1e4 / sigma_range_2 > 100 and sigma_range_2 > 0."""
    def fast(s):
        s2 = _F32(2.0) * (s * s)
        return bool(_F32(1e4) / s2 > _F32(100.0)) and bool(s2 > _F32(0.0))
    lo, hi = int(np.array(7.0, _F32).view(np.uint32)), int(np.array(7.2, _F32).view(np.uint32))
    as_f32 = lambda bits: np.array(bits, np.uint32).view(_F32)[()]   # noqa: E731
    assert fast(as_f32(lo)) and not fast(as_f32(hi))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fast(as_f32(mid)) else (lo, mid)
    return as_f32(lo), as_f32(hi)


UNIFORM_EDGES = ([("sigma_range", v) for v in ("fast max", "fast max + 1 ulp", 0.0, -1.5, np.nan, np.inf)] +
                 [("sigma_distance", v) for v in (0.0, 1e-30, np.nan, np.inf)] +
                 [("albedo_factor", v) for v in (0.0, -1.0, 2.0, np.nan)])


@pytest.mark.parametrize("name,value", UNIFORM_EDGES, ids=[f"{n}={v}" for n, v in UNIFORM_EDGES])
def test_denoise_uniform_edges_equal_the_oracle(O, frames, name, value):
    """Uniforms at and beyond the edges of what the kernels assume, in exact mode through both kernels: the oracle's image bit for
    bit (the API takes any binary32 for them; only radius > 8 is refused)."""
    if isinstance(value, str):
        lo, hi = fast_sigma_range_edge()
        assert hi == np.nextafter(lo, _F32(np.inf)) and 7.0 < lo < 7.1
        value = lo if value == "fast max" else hi
    f = frames(97, 49)
    for radius in (2, 7):
        uniforms = {name: float(value)}
        want = f.oracle(O, radius, **uniforms)
        for mode in (0, 2):
            assert_bits_equal(f.denoise(radius, mode, **uniforms), want, f"{name} = {value!r}, radius {radius}, mode {mode}")


BAND_LAYOUTS = {1: (2, 16), 2: (3, 32), 3: (2, 48), 4: (3, 16), 5: (2, 32), 6: (3, 48), 7: (2, 16), 8: (3, 32)}   # radius -> (ranks, band rows)
TOLERANT_HALO_RADII = (3, 7)


@pytest.mark.parametrize("radius", PAIR_RADII, ids=[f"r{r}" for r in PAIR_RADII])
def test_halo_rows_at_every_radius(O, H, scenes, noise, radius):
    """Row bands over 2 or 3 contexts, exotic pixels on the band edges and in the deepest halo row, in the left columns only (the right
    blocks stay lean): the stitched output with the stage whole and split around the exchange equals the oracle bit for bit in exact
    mode (both kernels), and in tolerant mode passes the sweep's checks."""
    from gpu_voxel_raytracer_amd import (DENOISE, DENOISE_EDGE, DENOISE_INTERIOR, DENOISED, NORMAL_DEPTH, SAMPLED_COLOR, ALBEDO_NODE, TRACE,
                                         Camera, Context)
    nranks, band = BAND_LAYOUTS[radius]
    w, h = 96, 200
    at = []
    for e in range(band, h, band):
        for k, y in enumerate((e - radius, e - 1, e, e + radius - 1)):   # halo rows of the ranks on either side, and the band edge rows
            at += [(y, 3 + 7 * k), (y, 30 + k)]
    color, nd, alb = planned_gbuffer(w, h, seed=1000 * radius + band, exotic_at=at)
    exotic = exotic_pixels(color, nd)
    assert exotic.sum() == len(set(at))
    pos, mrgb, size = scenes.load_scene("8x8x8")
    cam = scenes.bench_camera(size)
    want = oracle_denoise(O, color, nd, alb, cam, radius)
    assert np.isnan(want[..., :3]).any() and np.isfinite(want[..., :3]).mean() > 0.4
    rt = hip()
    rt.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    rt.hipFree.argtypes = [C.c_void_p]
    ctxs = [Context(w, h, max_bounces=1, noise=noise, rank=r, nranks=nranks, band_rows=band) for r in range(nranks)]
    bufs = []
    try:
        rows = []
        for c in ctxs:
            c.recreate_octree(pos, mrgb)
            c.camera = Camera(*cam)
            c.render(TRACE)
            c.sync()
            rr = c.local_rows()
            rows.append(rr)
            assert_both_paths(exotic, radius, f"rank {len(rows) - 1} of {nranks}, radius {radius}", rows=rr)
            for which, img in ((SAMPLED_COLOR, color), (NORMAL_DEPTH, nd), (ALBEDO_NODE, alb)):
                ptr, nbytes = c.device_image(which)
                mine = np.ascontiguousarray(img[rr])
                assert nbytes == mine.nbytes
                assert rt.hipMemcpy(C.c_void_p(ptr), mine.ctypes.data_as(C.c_void_p), nbytes, 1) == 0
            c.denoise_uniforms.radius = radius
            c.update_bindings()
            p, n = C.c_void_p(), C.c_void_p()
            assert rt.hipMalloc(C.byref(p), c.halo_bytes()) == 0
            bufs.append(p)
            assert rt.hipMalloc(C.byref(n), c.halo_bytes()) == 0
            bufs.append(n)
        assert any(not careful_blocks(exotic, radius, rr).all() for rr in rows)
        for mode in (0, 2) + ((1,) if radius in TOLERANT_HALO_RADII else ()):
            for split in (False, True):
                for c in ctxs:
                    c.set_option(H.OPT_DENOISE_MODE, mode)
                for r, c in enumerate(ctxs):
                    c.halo_export(bufs[2 * r].value, bufs[2 * r + 1].value)
                    if split:
                        c.render_stage(DENOISE_INTERIOR)
                got = np.zeros_like(want)
                for r, c in enumerate(ctxs):
                    c.halo_import(bufs[2 * ((r - 1) % nranks) + 1].value, bufs[2 * ((r + 1) % nranks)].value)
                    c.render_stage(DENOISE_EDGE if split else DENOISE)
                    got[rows[r]] = c.read(DENOISED)
                what = f"{nranks} ranks, {band}-row bands, radius {radius}, mode {mode}, {'split' if split else 'whole'}"
                if mode == 1:
                    assert_tolerant_close(got, want, what, exotic=exotic)
                else:
                    assert_bits_equal(got, want, what)
    finally:
        for c in ctxs:
            c.close()
        for p in bufs:
            rt.hipFree(p)
