"""GPU: the octree depth of a loaded scene changed in place (include/vxrt_scene_depth.h).  After every call the device records equal the
model's (tests/scene_depth_model.py) byte for byte; the voxels, their read-back order and the picks stay; and whenever the scene's
depth is what a rebuild of its voxels would give, every image of every frame is bit-identical to that rebuild's — for tracers 1 and 4,
the sky cull on and off, several frames in flight and per launch.  Edits and grid edits past the old root cube work after a grow."""
import ctypes as C

import numpy as np
import pytest
import torch   # before the first context: one HIP runtime in the process (host.py: set_voxels_device)

import edit_model as M
import scene_depth_model as SD
import scene_invariants as SI
from conftest import assert_bits_equal, require_variants
from test_gpu_edit import CONFIGS, H_, SCENES, W, assert_same_frames, base_scene, batches, fresh, make_ctx, trace_images

pytestmark = pytest.mark.gpu


class Tracked:
    """A context's scene and the counts it was loaded with (the build counts of the storage rule: the first edit or depth change
    takes them, and nothing changes the counts before that)."""

    def __init__(self, ctx):
        self.ctx = ctx
        svo, leaves = ctx.read_scene()
        self.built = (len(svo), len(leaves))

    def model(self):
        svo, leaves = self.ctx.read_scene()
        return SD.Scene(svo, leaves, self.ctx.scene_depth, built=self.built, live=self.ctx.stats().octree_nodes)

    def call(self, depth=None):
        """set_scene_depth(depth), or fit_scene_depth() with depth None, checked against the model."""
        s = self.model()
        if depth is None:
            got = self.ctx.fit_scene_depth()
            assert got == SD.fit(s)
        else:
            self.ctx.set_scene_depth(depth)
            SD.set_depth(s, depth)
        svo, leaves = self.ctx.read_scene()
        want_svo, want_leaves = s.arrays()
        assert np.array_equal(svo, want_svo) and np.array_equal(leaves, want_leaves), "device records differ from the model's"
        assert self.ctx.scene_depth == s.depth and self.ctx.stats().octree_nodes == s.live
        return s.depth


def listed(ctx):
    return M.from_list(*ctx.get_voxels())


def check_rebuild(H, ctx, model, cam, cfg, frame, what, also=None):
    """ctx holds `model` at the depth its rule gives: decoded list, read-back, node count and frames equal a fresh build's.
    also(ref): what else the caller compares with the fresh build while it is loaded."""
    pos, mrgb = M.to_list(model)
    assert ctx.scene_depth == H.scene_depth_for(pos), what
    assert M.decode_records(*ctx.read_scene(), ctx.scene_depth) == model, what
    assert listed(ctx) == model, what
    with fresh(H, cfg, model, cam) as ref:
        assert ref.stats().octree_depth == ctx.scene_depth
        assert ctx.stats().octree_nodes == ref.stats().octree_nodes, what
        assert_same_frames(H, ctx, ref, cfg, frame, what)
        if also is not None:
            also(ref)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "tracer%d-cull%d-fif%d-fpl%d" % c)
@pytest.mark.parametrize("name", SCENES)
def test_grow_then_edit_past_the_old_cube_equals_a_rebuild(H, scenes, name, cfg):
    load, model, cam, depth = base_scene(H, scenes, name)
    with make_ctx(H, cfg) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        t = Tracked(ctx)
        order = ctx.get_voxels()[0]
        assert t.call(depth + 1) == depth + 1
        assert np.array_equal(ctx.get_voxels()[0], order), "read-back order after a grow"
        lim = 1 << (depth + 1)
        # one voxel past the grown cube: edit_voxels(grow=True) grows once more
        far = np.array([[lim, 1, 2], [3, lim + 1, -lim]], np.int16)
        ctx.edit_voxels(far, [[1, 200, 30, 40], [0, 10, 220, 30]], grow=True)
        M.apply(model, far, [[1, 200, 30, 40], [0, 10, 220, 30]])
        assert ctx.scene_depth == depth + 2
        check_rebuild(H, ctx, model, cam, cfg, 3, f"{name}: edit_voxels(grow=True)")
        # a grid past that cube (SET): edit_voxel_grid(grow=True) grows again
        g = torch.zeros((2, 3, 2), dtype=torch.int32, device=f"cuda:{ctx.device}")
        g[0, 0, 0], g[1, 2, 1] = int(np.int32(np.uint32(0x81A0B0C0))), int(np.int32(np.uint32(0x80102030)))
        origin = (-(2 * lim) - 2, 0, 5)
        ctx.edit_voxel_grid(g, origin, mode="set", grow=True)
        M.apply(model, [[origin[0], 0, 5], [origin[0] + 1, 2, 6]], [[1, 0xA0, 0xB0, 0xC0], [0, 0x10, 0x20, 0x30]])
        assert ctx.scene_depth == depth + 3
        check_rebuild(H, ctx, model, cam, cfg, 5, f"{name}: edit_voxel_grid(grow=True)")
        # clear what lies past the first cube: the fit goes back to the build's depth
        M.apply(model, far, None)
        ctx.clear_voxels(far)
        ctx.edit_voxel_grid(g, origin, mode="clear")
        M.apply(model, [[origin[0], 0, 5], [origin[0] + 1, 2, 6]], None)
        assert t.call() == depth
        check_rebuild(H, ctx, model, cam, cfg, 7, f"{name}: fit after clears")


def test_pure_growth_keeps_the_list_the_picks_and_the_frames(H, scenes):
    cfg = (4, 1, 2, 8)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    with make_ctx(H, cfg) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        t = Tracked(ctx)
        pos0, mrgb0 = ctx.get_voxels()
        xs, ys = np.meshgrid(np.arange(0, W, 4), np.arange(0, H_, 4))
        picks = ctx.pick_pixels(xs.ravel(), ys.ravel())
        assert (picks["status"] == 1).any()
        for k, target in enumerate((depth + 1, depth + 4, 15)):
            assert t.call(target) == target
            pos, mrgb = ctx.get_voxels()
            assert np.array_equal(pos, pos0) and np.array_equal(mrgb, mrgb0), target
            got = ctx.pick_pixels(xs.ravel(), ys.ravel())
            for key in ("status", "voxel", "leaf"):
                assert np.array_equal(got[key], picks[key]), (target, key)
            # the twin: the list plus a far voxel that pins the depth, which the twin then clears (same list, same depth)
            anchor = np.array([[-(1 << target)] * 3], np.int16)
            with fresh(H, cfg, M.apply(dict(model), anchor, [[0, 1, 1, 1]]), cam) as twin:
                twin.clear_voxels(anchor)
                assert twin.stats().octree_depth == target
                assert twin.stats().octree_nodes == ctx.stats().octree_nodes
                assert_same_frames(H, ctx, twin, cfg, 3 + 2 * k, f"grown to {target}")


@pytest.mark.parametrize("name", ["menger", "empty", "minus_one"])
def test_shrink_and_fit_after_clearing_the_far_voxels(H, scenes, name):
    cfg = (1, 1, 1, 1)
    if name == "menger":
        _, model, cam, _ = base_scene(H, scenes, "menger")
    else:
        model = {} if name == "empty" else {(-1, -1, -1): M.word((2, 250, 200, 100))}
        cam = ((0.3, 0.4, -3.0), (0.0, 0.0, 1.0), 1.0)
    far = np.array([[-32768, 0, 7], [32767, 32767, -5], [5, -32768, 32767]], np.int16)
    with make_ctx(H, cfg) as ctx:
        ctx.recreate_octree(*M.to_list(M.apply(dict(model), far, [[1, 9, 9, 9]] * 3)))
        ctx.camera = H.Camera(*cam)
        assert ctx.scene_depth == 15
        t = Tracked(ctx)
        ctx.clear_voxels(far)
        want = H.scene_depth_for(M.to_list(model)[0])
        assert want == {"menger": 7, "empty": 0, "minus_one": 1}[name]
        assert t.call() == want
        check_rebuild(H, ctx, model, cam, cfg, 2, f"{name}: fit")
        assert t.call(15) == 15
        assert t.call(want) == want
        check_rebuild(H, ctx, model, cam, cfg, 4, f"{name}: 15 and back")


def test_random_edits_after_growing_an_edited_scene_equal_rebuilds(H, scenes):
    """The storage rule: the root's children block of an edited scene lies beyond the build counts, so a grow that let its new nodes
    share it would let the next widening edit run over a sibling."""
    cfg = (4, 0, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "castle")
    contexts = [make_ctx(H, cfg), make_ctx(H, cfg)]
    try:
        for c in contexts:
            load(c)
            c.camera = H.Camera(*cam)
        tracked = [Tracked(c) for c in contexts]
        anchor = np.array([[-(1 << depth)] * 3], np.int16)
        for label, pos, mrgb in list(batches(model, depth, seed=13))[:2] + [("anchor", anchor, [[3, 40, 50, 60]])]:
            for c in contexts:
                (c.clear_voxels(pos) if mrgb is None else c.edit_voxels(pos, mrgb))
            M.apply(model, pos, mrgb)
        grown = depth + 2
        for t in tracked:
            assert t.call(grown) == grown
        assert SD.block_owners(tracked[0].model())
        SI.check(*contexts[0].read_scene(), grown, contexts[0].scene_storage(), contexts[0].stats().octree_nodes, built=tracked[0].built)
        anchor = np.array([[-(1 << grown)] * 3], np.int16)       # pins every rebuild below at the grown depth
        for c in contexts:
            c.edit_voxels(anchor, [[3, 40, 50, 60]])
        M.apply(model, anchor, [[3, 40, 50, 60]])
        for k, (label, pos, mrgb) in enumerate(batches(model, grown, seed=17)):
            for c in contexts:
                (c.clear_voxels(pos) if mrgb is None else c.edit_voxels(pos, mrgb))
            M.apply(model, pos, mrgb)
            a, b = contexts[0].read_scene(), contexts[1].read_scene()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two contexts, same calls: same records"
            assert M.decode_records(*a, grown) == model, label
            if k % 3 == 0 or k == 7:
                check_rebuild(H, contexts[0], model, cam, cfg, 3 + 2 * k, f"after growth: {label}")
    finally:
        for c in contexts:
            c.close()


def test_history_is_kept_across_a_grow(H, O, scenes, noise):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "castle")
    with H.Context(W, H_, max_bounces=3, tracer=4, noise=noise) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        for f in (1, 2):
            ctx.set_frame_number(f)
            ctx.render(H.ALL)
        old_c, old_nd = ctx.read(H.ACCUM_COLOR), ctx.read(H.NORMAL_DEPTH)
        ctx.set_scene_depth(depth + 3)
        ctx.set_frame_number(3)
        ctx.render(H.ALL)
        u = O.Uniforms.default()
        u.set_camera(cam[0], O.camera_axis_scaled(cam[0], cam[1], cam[2], W, H_))
        cam16 = u.camera16()
        want = O.temporal(ctx.read(H.SAMPLED_COLOR), ctx.read(H.NORMAL_DEPTH), old_c, old_nd, cam16, cam16, O.Temporal.default(), True)
        assert_bits_equal(ctx.read(H.ACCUM_COLOR), want, "accumulated colour after a grow")
        fresh_hist = O.temporal(ctx.read(H.SAMPLED_COLOR), ctx.read(H.NORMAL_DEPTH), old_c, old_nd, cam16, cam16, O.Temporal.default(), False)
        assert not np.array_equal(want, fresh_hist), "the check must tell kept history from none"


def test_refusals_change_nothing(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    with make_ctx(H, cfg) as empty:
        for call in (lambda: empty.set_scene_depth(3), empty.fit_scene_depth):
            with pytest.raises(H.VxrtError) as e:
                call()
            assert e.value.status == H.E_NOSCENE
    with make_ctx(H, cfg) as ctx, make_ctx(H, cfg) as ref:
        for c in (ctx, ref):
            load(c)
            c.camera = H.Camera(*cam)
        ctx.set_scene_depth(depth + 2)
        ref.set_scene_depth(depth + 2)
        before = ctx.read_scene()
        for bad, status in ((depth - 1, H.E_SCENE), (0, H.E_SCENE), (16, H.E_INVALID), (1 << 31, H.E_INVALID)):
            with pytest.raises(H.VxrtError) as e:
                ctx.set_scene_depth(bad)
            assert e.value.status == status, bad
        assert ctx._L.vxrt_set_scene_depth(None, C.c_uint32(3)) == H.E_INVALID
        after = ctx.read_scene()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and ctx.scene_depth == depth + 2
        for i, (a, b) in enumerate(zip(trace_images(H, ctx, cfg, 2), trace_images(H, ref, cfg, 2))):
            assert_bits_equal(a, b, f"after refusals: image {i}")
    pos, mrgb, _ = scenes.load_scene("castle")
    with make_ctx(H, (1, 1, 1, 1), tuning=[(H.OPT_NODE_ORDER, 2)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        assert ctx.stats().node_order == 2
        before = ctx.read_scene()
        for call in (lambda: ctx.set_scene_depth(ctx.scene_depth + 1), ctx.fit_scene_depth):
            with pytest.raises(H.VxrtError) as e:
                call()
            assert e.value.status == H.E_INVALID
        after = ctx.read_scene()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_wide_record_scenes_are_refused(H, scenes):
    require_variants(H, wide=1)
    pos, mrgb, size = scenes.load_scene("menger")
    with H.Context(W, H_, tuning=[(H.OPT_SCENE_FORMAT, 1)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        assert ctx.stats().scene_format == 1
        d = ctx.scene_depth
        for call in (lambda: ctx.set_scene_depth(d + 1), ctx.fit_scene_depth):
            with pytest.raises(H.VxrtError) as e:
                call()
            assert e.value.status == H.E_INVALID
        assert ctx.scene_depth == d


def test_two_ranks_make_the_same_calls(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "castle")
    far = np.array([[1 << depth, 3, 3]], np.int16)
    with make_ctx(H, cfg) as single:
        ranks = [H.Context(W, H_, max_bounces=3, tracer=4, rank=r, nranks=2, band_rows=16) for r in range(2)]
        try:
            for c in [single] + ranks:
                load(c)
                c.camera = H.Camera(*cam)
                c.set_scene_depth(depth + 2)
                c.edit_voxels(far, [[1, 255, 0, 0]], grow=True)
                c.clear_voxels(far)
                assert c.fit_scene_depth() == depth
                c.set_frame_number(6)
                c.render(H.TRACE)
            full = single.read(H.SAMPLED_COLOR)
            for c in ranks:
                assert_bits_equal(c.read(H.SAMPLED_COLOR), full[c.local_rows()], "rank rows")
                a, b = c.read_scene(), single.read_scene()
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        finally:
            for c in ranks:
                c.close()
