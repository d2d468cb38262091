"""GPU: building a scene on the device from a voxel list in device memory (include/vxrt_device_scene.h).  Every comparison is bit for
bit: the device's records and leaf words (vxrt_debug_read_scene) equal the host builder's (vxrt_build_records) and the Python model's
(tests/device_build_model.py); stats, frames, edits, read-back and picks equal those of a context given the same list by
vxrt_set_voxels; lists past the host builder's node limit build; refused calls change nothing; a producer on another stream is
ordered by the Python wrapper."""
import ctypes as C
import time

import numpy as np
import pytest
# torch's HIP runtime must be the process's first: imported here, at collection, before any test loads libvxrt.so (as bench.py and
# the distributed workers import torch before the library)
import torch

import device_build_model as D
import extract_model as X
from conftest import assert_bits_equal, reference_vox, reference_vox_names, require_variants
from test_gpu_edit import CONFIGS, W, H_, assert_same_frames, make_ctx, pipeline_images, trace_images

pytestmark = pytest.mark.gpu

MRGB0 = (0, 0xB0, 0xD0, 0x60)
STATS = ("octree_depth", "octree_nodes", "scene_bytes", "wide_nodes", "cull_box_valid")


def assert_same_scene(a, b, what=""):
    sa, la = a.read_scene()
    sb, lb = b.read_scene()
    assert np.array_equal(sa, sb), f"{what}: records"
    assert np.array_equal(la, lb), f"{what}: leaf words"
    ta, tb = a.stats(), b.stats()
    for f in STATS:
        assert getattr(ta, f) == getattr(tb, f), (what, f, getattr(ta, f), getattr(tb, f))
    assert list(ta.cull_box_min) == list(tb.cull_box_min) and list(ta.cull_box_max) == list(tb.cull_box_max), what


def assert_records(H, ctx, pos, mrgb, what=""):
    svo, _, leaves, depth = H.build_records(pos, mrgb)
    got_svo, got_leaves = ctx.read_scene()
    if len(leaves) == 0:
        leaves = np.zeros(1, np.int32)   # the empty scene's one zero leaf word (upload_svo)
    assert ctx.stats().octree_depth == depth, what
    assert np.array_equal(got_svo, svo), f"{what}: records"
    assert np.array_equal(got_leaves, leaves), f"{what}: leaf words"


def both(H, pos, mrgb, cfg=(1, 1, 1, 1), tuning=()):
    """-> (device-built context, host-built context) of the same list"""
    dev, host = make_ctx(H, cfg, tuning), make_ctx(H, cfg, tuning)
    dev.set_voxels_device(pos, mrgb)
    host.recreate_octree(pos, mrgb)
    return dev, host


@pytest.mark.parametrize("name", reference_vox_names() + ["startup"])
def test_fixture_scenes_equal_the_host_build(H, name):
    if name == "startup":
        pos, mrgb = H.default_scene_voxels(1)
    else:
        pos, mrgb, _ = H.vox_to_voxels(reference_vox(name))
    dev, host = both(H, pos, mrgb)
    with dev, host:
        assert_records(H, dev, pos, mrgb, name)
        assert_same_scene(dev, host, name)


def random_list(rng, n, lim):
    pos = rng.integers(-lim, lim, (n, 3)).astype(np.int16)
    pos = np.concatenate([pos, pos[rng.integers(0, n, n // 3)]])          # duplicates with other words
    mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    order = rng.permutation(len(pos))
    return pos[order], mrgb[order]


@pytest.mark.parametrize("lim", [1, 2, 9, 100, 3000, 32768])
def test_random_lists_with_duplicates_in_both_orders(H, lim):
    rng = np.random.default_rng(lim)
    pos, mrgb = random_list(rng, 200000, lim)
    with H.Context(W, H_) as ctx:
        for p, m, what in ((pos, mrgb, "shuffled"), (pos[::-1].copy(), mrgb[::-1].copy(), "reversed")):
            ctx.set_voxels_device(p, m)
            assert_records(H, ctx, p, m, f"lim {lim} {what}")
            svo, leaves, depth = D.build(p, m)
            assert np.array_equal(ctx.read_scene()[0], svo)


@pytest.mark.parametrize("depth", range(16))
def test_every_depth(H, depth):
    rng = np.random.default_rng(depth)
    lim = 1 << depth
    pos = np.concatenate([rng.integers(-lim, lim, (5000, 3)), [[lim - 1, -lim, 0]]]).astype(np.int16)
    mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    with H.Context(W, H_) as ctx:
        ctx.set_voxels_device(pos, mrgb)
        assert_records(H, ctx, pos, mrgb, f"depth {depth}")
        ctx.set_voxels_device(pos[-1:], mrgb[-1:])                             # one voxel
        assert_records(H, ctx, pos[-1:], mrgb[-1:], f"depth {depth}, n = 1")


def test_empty_list_equals_the_host(H):
    empty_p, empty_m = np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    dev, host = both(H, *H.default_scene_voxels(1))
    with dev, host:
        dev.set_voxels_device(empty_p, empty_m)
        host.recreate_octree(empty_p, empty_m)
        assert_records(H, dev, empty_p, empty_m, "empty")
        assert_same_scene(dev, host, "empty")
        assert_same_frames(H, dev, host, (1, 1, 1, 1), 3, "empty")


def test_deterministic_and_order_independent(H):
    rng = np.random.default_rng(7)
    pos = np.unique(rng.integers(-700, 700, (300000, 3)).astype(np.int16), axis=0)
    mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    with H.Context(W, H_) as ctx:
        ctx.set_voxels_device(pos, mrgb)
        first = ctx.read_scene()
        ctx.set_voxels_device(pos, mrgb)
        again = ctx.read_scene()
        perm = rng.permutation(len(pos))
        ctx.set_voxels_device(pos[perm], mrgb[perm])                           # no duplicates: the order cannot matter
        permuted = ctx.read_scene()
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    for a, b in zip(first, permuted):
        assert np.array_equal(a, b)


def scene_list(H, scenes, name):
    if name == "menger":
        return H.menger_voxels(3, MRGB0) + (scenes.close_camera((27, 27, 27)),)
    pos, mrgb = H.default_scene_voxels(1)
    return pos, mrgb, scenes.reference_start_camera()


def moving_frames(H, dev, host, cfg, cam, what, frames=3):
    for f in range(frames):
        c = H.Camera(np.asarray(cam[0], np.float32) + np.float32(0.37 * f), cam[1], cam[2])
        dev.camera = host.camera = c
        assert_same_frames(H, dev, host, cfg, 5 + f, f"{what} frame {f}")


@pytest.mark.parametrize("name", ["menger", "startup"])
@pytest.mark.parametrize("cfg", CONFIGS)
def test_frames_equal_the_host_build_after_a_previous_scene(H, name, cfg):
    from gpu_voxel_raytracer_amd import scenes
    pos, mrgb, cam = scene_list(H, scenes, name)
    dev, host = make_ctx(H, cfg), make_ctx(H, cfg)
    with dev, host:
        for c in (dev, host):                                                 # a previous scene with a temporal history
            c.set_menger(2, 0, (0, 200, 10, 10))
            c.camera = H.Camera(*cam)
            c.render(H.ALL)
        dev.set_voxels_device(pos, mrgb)
        host.recreate_octree(pos, mrgb)
        assert_same_scene(dev, host, name)
        moving_frames(H, dev, host, cfg, cam, f"{name} {cfg}")


@pytest.mark.parametrize("tracer", [2, 3, 5])
def test_frames_of_the_variant_tracers(H, tracer):
    require_variants(H, tracer=tracer)
    from gpu_voxel_raytracer_amd import scenes
    for name in ("menger", "startup"):
        pos, mrgb, cam = scene_list(H, scenes, name)
        for cull in (0, 1):
            cfg = (tracer, cull, 1, 1)
            dev, host = both(H, pos, mrgb, cfg)
            with dev, host:
                moving_frames(H, dev, host, cfg, cam, f"{name} tracer {tracer} cull {cull}", frames=2)


@pytest.mark.parametrize("order", [2, 3])
def test_node_order_options(H, order):
    from gpu_voxel_raytracer_amd import scenes
    for name in ("menger", "startup"):
        pos, mrgb, cam = scene_list(H, scenes, name)
        dev, host = both(H, pos, mrgb, tuning=[(H.OPT_NODE_ORDER, order)])
        with dev, host:
            assert dev.stats().node_order == host.stats().node_order
            assert_same_scene(dev, host, f"{name} order {order}")
            moving_frames(H, dev, host, (1, 1, 1, 1), cam, f"{name} order {order}", frames=2)


def test_wide_scene_format(H):
    require_variants(H, wide=1)
    from gpu_voxel_raytracer_amd import scenes
    for name in ("menger", "startup"):
        pos, mrgb, cam = scene_list(H, scenes, name)
        dev, host = both(H, pos, mrgb, tuning=[(H.OPT_SCENE_FORMAT, 1)])
        with dev, host:
            assert dev.stats().wide_nodes == host.stats().wide_nodes > 0
            assert_same_scene(dev, host, f"{name} wide")
            moving_frames(H, dev, host, (1, 1, 1, 1), cam, f"{name} wide", frames=2)


def test_edit_read_back_and_pick_after_the_build(H):
    from gpu_voxel_raytracer_amd import scenes
    pos, mrgb, cam = scene_list(H, scenes, "startup")
    dev, host = both(H, pos, mrgb)
    with dev, host:
        for c in (dev, host):
            c.camera = H.Camera(*cam)
        assert all(np.array_equal(a, b) for a, b in zip(dev.get_voxels(), host.get_voxels()))
        rng = np.random.default_rng(3)
        lim = 1 << dev.stats().octree_depth
        ep = rng.integers(-lim, lim, (500, 3)).astype(np.int16)
        em = rng.integers(0, 256, (500, 4)).astype(np.uint8)
        for c in (dev, host):
            c.edit_voxels(ep, em)
            c.clear_voxels(pos[::7])
        assert_same_scene(dev, host, "after edits")
        assert all(np.array_equal(a, b) for a, b in zip(dev.get_voxels(), host.get_voxels()))
        xs, ys = rng.integers(0, W, 200), rng.integers(0, H_, 200)
        pa, pb = dev.pick_pixels(xs, ys), host.pick_pixels(xs, ys)
        for k in pa:
            assert np.array_equal(pa[k].view(np.uint8), pb[k].view(np.uint8)), k
        assert_same_frames(H, dev, host, (1, 1, 1, 1), 9, "after edits")


def round_trip(H, menger, **ctx_kw):
    with H.Context(W, H_, **ctx_kw) as src:
        src.set_menger(*menger)
        want = src.read_scene()
        pos, mrgb = src.get_voxels()
    with H.Context(W, H_, **ctx_kw) as dst:
        t0 = time.perf_counter()
        dst.set_voxels_device(pos, mrgb)
        took = time.perf_counter() - t0
        got = dst.read_scene()
    assert np.array_equal(got[0], want[0]), "records"
    assert np.array_equal(got[1], want[1]), "leaf words"
    return len(pos), took


def test_round_trip_of_the_device_sponge(H):
    round_trip(H, (4, 70, MRGB0, 5))


def test_round_trip_at_config5_size(H):
    """config 5's 975 M voxels: get_voxels -> upload -> set_voxels_device gives set_menger's 5.99 GB of records byte for byte
    (under 6 s on one MI355X, most of it the host copies of the list and of the records)."""
    from gpu_voxel_raytracer_amd.scenes import CONFIG5
    n, took = round_trip(H, CONFIG5)
    assert n == X.menger_count(CONFIG5[0], CONFIG5[1])
    print(f"config 5: {n} voxels, upload + device build {took:.3f} s")


def test_beyond_the_host_node_limit(H):
    rng = np.random.default_rng(11)
    pos = rng.integers(-32768, 32768, (12_000_000, 3)).astype(np.int16)
    mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    assert D.depth_of(pos) == 15
    svo, leaves, depth = D.build(pos, mrgb)
    assert len(svo) >= 1 << 26
    with H.Context(W, H_) as ctx:
        ctx.set_menger(2, 0, MRGB0)
        with pytest.raises(H.VxrtError) as e:
            ctx.recreate_octree(pos, mrgb)
        assert e.value.status == H.E_SCENE
        ctx.set_voxels_device(pos, mrgb)
        got_svo, got_leaves = ctx.read_scene()
        assert np.array_equal(got_svo, svo)
        assert np.array_equal(got_leaves, leaves)
        assert ctx.stats().octree_nodes == len(svo)
        key = X.path_key(pos, depth)
        order = np.argsort(key, kind="stable")
        last = np.r_[key[order][1:] != key[order][:-1], True]
        gp, gm = ctx.get_voxels()
        assert np.array_equal(gp, pos[order][last])
        assert np.array_equal(gm, X.mrgb_of(leaves))


def test_refused_calls_change_nothing(H):
    from gpu_voxel_raytracer_amd import scenes
    pos, mrgb, cam = scene_list(H, scenes, "startup")
    cfg = (4, 1, 1, 1)
    ctx, ref = make_ctx(H, cfg), make_ctx(H, cfg)
    with ctx, ref:
        for c in (ctx, ref):
            c.set_voxels_device(pos, mrgb)
            c.camera = H.Camera(*cam)
            c.render(H.ALL)
        before = ctx.read_scene()
        L = ctx._L
        hp = np.ascontiguousarray(pos, np.int16)
        hm = np.ascontiguousarray(mrgb, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
        calls = [(None, None), (p(hp), None), (None, p(hm)), (p(hp), p(hm))]           # null arrays; numpy host memory
        for a, b in calls:
            assert L.vxrt_set_voxels_device(ctx._h, a, b, C.c_size_t(len(hp))) == H.E_INVALID
            after = ctx.read_scene()
            assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
        assert_same_scene(ctx, ref, "refused")
        for i, (a, b) in enumerate(zip(trace_images(H, ctx, cfg, 4), trace_images(H, ref, cfg, 4))):
            assert_bits_equal(a, b, f"refused: trace image {i}")
        for i, (a, b) in enumerate(zip(pipeline_images(H, ctx, cfg, 30), pipeline_images(H, ref, cfg, 30))):
            assert_bits_equal(a, b, f"refused: pipeline image {i}")


def test_producer_on_a_side_stream_is_ordered(H):
    rng = np.random.default_rng(5)
    pos = rng.integers(-300, 300, (400000, 3)).astype(np.int16)
    mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    dev = torch.device("cuda", 0)
    src_p, src_m = torch.as_tensor(pos, device=dev), torch.as_tensor(mrgb, device=dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(dev)
    with H.Context(W, H_) as ctx:
        with torch.cuda.stream(side):
            tp = torch.zeros_like(src_p)
            tm = torch.zeros_like(src_m)
            torch.cuda._sleep(50_000_000)           # the producer is still busy when the build is asked for
            tp.copy_(src_p)
            tm.copy_(src_m)
            ctx.set_voxels_device(tp, tm)
        assert_records(H, ctx, pos, mrgb, "side stream")
