"""GPU: an edited scene's octree compacted in place (include/vxrt_compact.h).  After vxrt_compact_scene the device records equal the
model's (tests/compact_model.py) applied to the read-back from before the call, byte for byte; the voxels, their read-back order,
the picks and every image stay; whenever the scene's depth is what a rebuild of its voxels would give, the records, the stats with
the sky-cull box and every frame equal a fresh build's; edits after a compaction equal edits after a fresh build; the temporal
history is kept; and a host that compacts keeps its storage bounded where one that does not grows with every clear-and-set cycle."""
import ctypes as C

import numpy as np
import pytest
import torch   # before the first context: one HIP runtime in the process (host.py: set_voxels_device)

import compact_model as CM
import edit_model as M
from conftest import assert_bits_equal, require_variants
from test_gpu_device_build import assert_same_scene
from test_gpu_edit import CONFIGS, H_, SCENES, W, assert_same_frames, base_scene, batches, fresh, make_ctx, trace_images

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FIELDS = ("records_live", "records_used", "records_capacity", "leaves_used", "leaves_capacity")


def same_arrays(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def assert_tight(ctx, what=""):
    """The storage of a fresh build: nothing but the live tree, allocated exactly."""
    st = ctx.scene_storage()
    assert sorted(st) == sorted(FIELDS)
    svo, leaves = ctx.read_scene()
    assert st["records_live"] == st["records_used"] == st["records_capacity"] == len(svo) == ctx.stats().octree_nodes, (what, st)
    assert st["leaves_used"] == st["leaves_capacity"] == len(leaves), (what, st)
    assert ctx.stats().scene_bytes == 8 * len(svo) + 4 * len(leaves), what
    return st


def compact_checked(ctx, what=""):
    """compact_scene() against the model applied to the read-back from before the call -> the arrays after it."""
    before, depth = ctx.read_scene(), ctx.scene_depth
    live = ctx.stats().octree_nodes
    ctx.compact_scene()
    after = ctx.read_scene()
    want = CM.compact(*before, depth)
    assert same_arrays(after, want), f"{what}: device records differ from the model's"
    assert ctx.scene_depth == depth and ctx.stats().octree_nodes == live == len(after[0]), what
    assert_tight(ctx, what)
    return after


def edited(H, scenes, name, cfg, seed=7):
    """A context holding `name` after test_gpu_edit's batch sequence (the anchor pins the depth of the model) -> (ctx, model, cam, depth)."""
    load, model, cam, depth = base_scene(H, scenes, name)
    ctx = make_ctx(H, cfg)
    load(ctx)
    ctx.camera = H.Camera(*cam)
    anchor = np.array([[-(1 << depth)] * 3], np.int16)
    ctx.edit_voxels(anchor, [[3, 40, 50, 60]])
    M.apply(model, anchor, [[3, 40, 50, 60]])
    apply_batches(ctx, model, depth, seed)
    return ctx, model, cam, depth


def apply_batches(ctx, model, depth, seed):
    for _, pos, mrgb in batches(model, depth, seed):
        (ctx.clear_voxels(pos) if mrgb is None else ctx.edit_voxels(pos, mrgb))
        M.apply(model, pos, mrgb)


def pixel_grid():
    xs, ys = np.meshgrid(np.arange(0, W, 4), np.arange(0, H_, 4))
    return xs.ravel(), ys.ravel()


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "tracer%d-cull%d-fif%d-fpl%d" % c)
@pytest.mark.parametrize("name", SCENES)
def test_compaction_is_byte_exact_and_changes_no_frame(H, scenes, name, cfg):
    ctx, model, cam, depth = edited(H, scenes, name, cfg)
    with ctx:
        st = ctx.scene_storage()
        assert st["records_used"] > st["records_live"] == ctx.stats().octree_nodes       # the edits left holes
        assert st["records_capacity"] >= st["records_used"] and st["leaves_capacity"] >= st["leaves_used"]
        assert ctx.stats().scene_bytes == 8 * st["records_capacity"] + 4 * st["leaves_capacity"]
        voxels, picks, images = ctx.get_voxels(), ctx.pick_pixels(*pixel_grid()), trace_images(H, ctx, cfg, 3)
        assert name != "menger" or (picks["status"] == 1).any()
        compact_checked(ctx, name)
        for a, b in zip(ctx.get_voxels(), voxels):
            assert np.array_equal(a, b), "get_voxels and its order"
        got = ctx.pick_pixels(*pixel_grid())
        for key in picks:
            assert np.array_equal(got[key].view(np.uint8), picks[key].view(np.uint8)), key
        for i, (a, b) in enumerate(zip(trace_images(H, ctx, cfg, 3), images)):
            assert_bits_equal(a, b, f"{name}: trace image {i} across the compaction")
        # the depth is the list's rule (the anchor): a fresh context given the list holds the same bytes
        assert ctx.scene_depth == H.scene_depth_for(M.to_list(model)[0]) == depth
        with fresh(H, cfg, model, cam) as ref:
            assert_same_scene(ctx, ref, f"{name}: compacted against a fresh build")
            assert ctx.scene_storage() == ref.scene_storage()
            assert_same_frames(H, ctx, ref, cfg, 5, f"{name}: compacted against a fresh build")


@pytest.mark.parametrize("cfg", [(4, 1, 1, 1), (1, 0, 2, 8)], ids=lambda c: "tracer%d-cull%d-fif%d-fpl%d" % c)
@pytest.mark.parametrize("name", ["castle", "menger_device"])
def test_edits_after_a_compaction_equal_edits_after_a_fresh_build(H, scenes, name, cfg):
    ctx, model, cam, depth = edited(H, scenes, name, cfg)
    with ctx:
        ctx.compact_scene()
        pos, mrgb = ctx.get_voxels()
        assert M.from_list(pos, mrgb) == model
        with make_ctx(H, cfg) as ref:
            ref.recreate_octree(pos, mrgb)
            ref.camera = H.Camera(*cam)
            assert_same_scene(ctx, ref, f"{name}: before the second sequence")
            for k, (label, p, c) in enumerate(batches(model, depth, seed=13)):
                for x in (ctx, ref):
                    (x.clear_voxels(p) if c is None else x.edit_voxels(p, c))
                M.apply(model, p, c)
                assert_same_scene(ctx, ref, f"{name}: {label} after a compaction")      # the storage rule started over
                assert ctx.scene_storage() == ref.scene_storage(), label
                if k % 3 == 1:
                    assert_same_frames(H, ctx, ref, cfg, 3 + 2 * k, f"{name}: {label} after a compaction")
            assert M.decode_records(*ctx.read_scene(), depth) == model
            st = ctx.scene_storage()
            assert st["records_used"] > st["records_live"]
            compact_checked(ctx, f"{name}: second compaction")
            assert not same_arrays(ctx.read_scene(), ref.read_scene())
            ref.compact_scene()
            assert_same_scene(ctx, ref, f"{name}: both compacted")


@pytest.mark.parametrize("cfg", [(4, 1, 1, 1), (4, 1, 2, 8)], ids=lambda c: "tracer%d-cull%d-fif%d-fpl%d" % c)
def test_history_is_kept_across_a_compaction(H, scenes, cfg):
    """The whole pipeline (trace, temporal, denoise) with a compaction in the middle equals the same run without it; a run that
    lost its history there does not."""
    def frames(ctx, n):
        if cfg[3] > 1:
            ctx.render_frames(H.ALL, cfg[3] * n)
        else:
            for _ in range(n):
                ctx.render(H.ALL)

    runs = [edited(H, scenes, "castle", cfg) for _ in range(3)]
    try:
        for ctx, _, _, _ in runs:
            ctx.set_frame_number(1)
            frames(ctx, 2)
        with_call, without, forgetful = (r[0] for r in runs)
        with_call.compact_scene()                 # drains the frames in flight, keeps the history
        forgetful.reset_history()
        for ctx in (with_call, without, forgetful):
            frames(ctx, 2)
        images = (H.SAMPLED_COLOR, H.NORMAL_DEPTH, H.ACCUM_COLOR, H.DENOISED)
        for i in images:
            assert_bits_equal(with_call.read(i), without.read(i), f"image {i} with a compaction in the middle")
        assert np.array_equal(with_call.read(H.DISPLAY_RGBA8_SRGB), without.read(H.DISPLAY_RGBA8_SRGB))
        assert not np.array_equal(forgetful.read(H.ACCUM_COLOR), without.read(H.ACCUM_COLOR)), "the check must tell kept history from none"
    finally:
        for r in runs:
            r[0].close()


def test_growth_is_bounded_by_compaction(H, scenes):
    """64 clear-and-set cycles of an aligned 16^3 box: every cycle prunes and recreates 1 + 8 + 64 inner nodes and 512 leaf parents,
    so without compaction the arrays in use grow by 73 x 8 records and 512 x 8 leaf words per cycle; with a compaction after each
    cycle the storage is the same five numbers, and the same bytes, after every cycle."""
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    assert depth >= 5
    box = np.array([(32 + x, 32 + y, 32 + z) for x, y, z in np.ndindex(16, 16, 16)], np.int16)
    assert (box.max() < (1 << depth)) and np.all((box.min(0) + (1 << depth)) % 16 == 0)
    colours = np.random.default_rng(9).integers(0, 256, (len(box), 4)).astype(np.uint8)
    with make_ctx(H, cfg) as leaky, make_ctx(H, cfg) as kept:
        for c in (leaky, kept):
            load(c)
            c.camera = H.Camera(*cam)
        seen, last, arrays = [], None, None
        for cycle in range(64):
            for c in (leaky, kept):
                c.clear_voxels(box)
                c.edit_voxels(box, colours)
            st = leaky.scene_storage()
            if last is not None:
                assert st["records_used"] == last["records_used"] + 73 * 8, (cycle, st, last)
                assert st["leaves_used"] == last["leaves_used"] + 512 * 8, (cycle, st, last)
                assert st["records_live"] == last["records_live"]
            last = st
            kept.compact_scene()
            seen.append(tuple(kept.scene_storage()[f] for f in FIELDS))
            if cycle in (0, 1, 63):
                now = kept.read_scene()
                assert arrays is None or same_arrays(now, arrays), cycle
                arrays = now
        assert len(set(seen)) == 1, sorted(set(seen))
        assert_tight(kept, "after 64 cycles")
        assert last["records_used"] > seen[0][1] + 62 * 73 * 8 and last["records_live"] == seen[0][0]
        M.apply(model, box, colours)
        assert M.decode_records(*leaky.read_scene(), depth) == model
        for i, (a, b) in enumerate(zip(trace_images(H, leaky, cfg, 4), trace_images(H, kept, cfg, 4))):
            assert_bits_equal(a, b, f"image {i}: with and without compaction")
        compact_checked(leaky, "the leaky one at last")
        assert same_arrays(leaky.read_scene(), arrays)


@pytest.mark.parametrize("name", ["castle", "menger_device"])
def test_compaction_after_depth_changes(H, scenes, name):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, name)
    with make_ctx(H, cfg) as each, make_ctx(H, cfg) as once, fresh(H, cfg, model, cam) as ref:
        for c in (each, once):
            load(c)
            c.camera = H.Camera(*cam)
        assert H.scene_depth_for(M.to_list(model)[0]) == depth
        steps = [("grow by 1", lambda c: c.set_scene_depth(depth + 1)), ("grow to 15", lambda c: c.set_scene_depth(15)),
                 ("shrink back", lambda c: c.set_scene_depth(depth + 1)), ("fit", lambda c: c.fit_scene_depth())]
        for label, step in steps:
            step(each)
            step(once)
            st = each.scene_storage()
            assert st["records_used"] > st["records_live"], label
            compact_checked(each, f"{name}: {label}")
            assert M.decode_records(*each.read_scene(), each.scene_depth) == model, label
            for i, (a, b) in enumerate(zip(trace_images(H, each, cfg, 2), trace_images(H, once, cfg, 2))):
                assert_bits_equal(a, b, f"{label}: image {i}, compacted or not")
        assert each.scene_depth == once.scene_depth == depth
        compact_checked(once, f"{name}: every step, then one compaction")
        for c in (each, once):
            assert_same_scene(c, ref, f"{name}: at the rule's depth")
        assert_same_frames(H, once, ref, cfg, 6, f"{name}: at the rule's depth")


def test_device_built_sponge_with_a_2_20_entry_device_edit(H, scenes):
    """The level-6 sponge (729^3, 64 M voxels: the largest the suite builds whose read-back the numpy model can hold; the level-7
    one is 5.6 GiB): the leaf parents' level and the three above it span thousands, hundreds and tens of 2048-entry blocks, so the
    scan runs over many partials.  A 2^20-entry device edit reallocates the never-edited storage; half of it is cleared again."""
    rng = np.random.default_rng(23)
    with H.Context(W, H_, max_bounces=2) as ctx:
        ctx.set_menger(6, 0, (0, 150, 170, 120), 4096)
        depth = ctx.scene_depth
        lim = 1 << depth
        assert depth == 10 and ctx.stats().octree_nodes > 2048 * 2048
        ext = np.float32(729 * 0.5)
        eye = (np.array([-0.45, 0.30, -0.55], np.float32) * ext + ext / 2).astype(np.float32)
        ctx.camera = H.Camera(eye, (np.full(3, ext / 2, np.float32) - eye).astype(np.float32), 1.2217305)
        assert_tight(ctx, "as built")
        built = ctx.read_scene()
        ctx.compact_scene()                                   # never edited: nothing to do
        assert same_arrays(ctx.read_scene(), built)
        del built
        n = 1 << 20
        pos = torch.as_tensor(rng.integers(-lim, lim, (n, 3)).astype(np.int16), device=DEV)
        mrgb = torch.as_tensor(rng.integers(0, 256, (n, 4)).astype(np.uint8), device=DEV)
        bytes_before = ctx.stats().scene_bytes
        ctx.edit_voxels_device(pos, mrgb)
        assert ctx.stats().scene_bytes > bytes_before                                    # the batch crossed a reallocation
        ctx.clear_voxels_device(pos[: n // 2])
        st = ctx.scene_storage()
        assert st["records_used"] > st["records_live"] + (1 << 20)
        count = ctx.count_voxels()
        ctx.set_frame_number(2)
        ctx.render(H.TRACE)
        images = [ctx.read(i) for i in (H.SAMPLED_COLOR, H.NORMAL_DEPTH)]
        compact_checked(ctx, "level-6 sponge")
        assert ctx.count_voxels() == count
        ctx.set_frame_number(2)
        ctx.render(H.TRACE)
        for i, want in zip((H.SAMPLED_COLOR, H.NORMAL_DEPTH), images):
            assert_bits_equal(ctx.read(i), want, f"image {i} across the compaction")
        # the rebuild route: the voxel list, extracted and built again on the device
        p, m = ctx.get_voxels_device()
        assert H.scene_depth_for([[int(p.min())] * 3, [int(p.max())] * 3]) == depth
        with H.Context(W, H_, max_bounces=2) as ref:
            ref.set_voxels_device(p, m)
            assert_same_scene(ctx, ref, "level-6 sponge against the device builder")


def small_scene(name):
    if name == "empty":
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    if name == "one voxel":
        return np.array([[-1, -1, -1]], np.int16), np.array([[1, 2, 3, 4]], np.uint8)
    assert name == "depth 0"
    return np.array([[0, 0, 0], [-1, 0, -1], [0, -1, 0]], np.int16), np.array([[1, 2, 3, 4], [0, 9, 8, 7], [2, 5, 5, 5]], np.uint8)


@pytest.mark.parametrize("name", ["empty", "one voxel", "depth 0"])
def test_small_scenes(H, scenes, name):
    cfg = (4, 1, 1, 1)
    pos, mrgb = small_scene(name)
    cam = ((0.3, 0.4, -3.0), (0.0, 0.0, 1.0), 1.0)
    model = M.from_list(pos, mrgb)
    with fresh(H, cfg, model, cam) as ctx, fresh(H, cfg, model, cam) as ref:
        depth = ctx.scene_depth
        assert depth == {"empty": 0, "one voxel": 1, "depth 0": 0}[name]
        built = ctx.read_scene()
        ctx.compact_scene()                                   # never edited
        assert same_arrays(ctx.read_scene(), built) and same_arrays(CM.compact(*built, depth), built)
        assert_tight(ctx, name)
        # every position of the root cube set, then those the scene does not hold cleared again: the same voxels, an edited layout
        lim = 1 << depth
        cube = np.array([np.array(p) - lim for p in np.ndindex(2 * lim, 2 * lim, 2 * lim)], np.int16)
        extra = np.array([p for p in cube.tolist() if tuple(p) not in model], np.int16).reshape(-1, 3)
        ctx.edit_voxels(extra, [[5, 1, 2, 3]] * len(extra))
        ctx.clear_voxels(extra)
        assert ctx.scene_storage()["records_capacity"] > len(built[0]) or ctx.scene_storage()["leaves_capacity"] > len(built[1])
        assert same_arrays(compact_checked(ctx, name), built)
        assert_same_scene(ctx, ref, name)
        assert_same_frames(H, ctx, ref, cfg, 3, name)
        # and an edit afterwards is an edit of a fresh build
        for c in (ctx, ref):
            c.edit_voxels(cube[:3], [[1, 200, 100, 50]] * 3)
        assert_same_scene(ctx, ref, f"{name}: edited after the compaction")


def test_a_scene_cleared_to_empty_by_edits(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "castle")
    with make_ctx(H, cfg) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        ctx.clear_voxels(np.array(sorted(model), np.int16))
        assert ctx.count_voxels() == 0 and ctx.scene_storage()["records_live"] == 1
        after = compact_checked(ctx, "cleared to empty")
        assert after[0].tolist() == [[0, 1]] and after[1].tolist() == [0]          # what vxrt_set_voxels holds for an empty list
        assert ctx.scene_depth == depth and not ctx.stats().cull_box_valid
        some = np.array(sorted(model)[:50], np.int16)
        ctx.edit_voxels(some, [[2, 9, 8, 7]] * len(some))
        assert M.decode_records(*ctx.read_scene(), depth) == M.from_list(some, [[2, 9, 8, 7]] * len(some))
        assert ctx.fit_scene_depth() == H.scene_depth_for(some)
        compact_checked(ctx, "set again")
        with fresh(H, cfg, M.from_list(some, [[2, 9, 8, 7]] * len(some)), cam) as ref:
            assert_same_scene(ctx, ref, "set again, fitted, compacted")
            assert_same_frames(H, ctx, ref, cfg, 3, "set again, fitted, compacted")


def test_the_cull_box_shrinks_to_a_fresh_builds(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    far = np.array([[-(1 << depth)] * 3, [(1 << depth) - 1] * 3], np.int16)
    with make_ctx(H, cfg) as ctx, fresh(H, cfg, model, cam) as ref:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        ctx.edit_voxels(far, [[1, 1, 1, 1]] * 2)
        ctx.clear_voxels(far)
        grown, want = ctx.stats(), ref.stats()
        assert list(grown.cull_box_min) != list(want.cull_box_min)                # edits only ever grow the box
        images = trace_images(H, ctx, cfg, 2)
        compact_checked(ctx, "far voxels set and cleared")
        assert_same_scene(ctx, ref, "the box of a fresh build")
        for i, (a, b) in enumerate(zip(trace_images(H, ctx, cfg, 2), images)):
            assert_bits_equal(a, b, f"image {i}: frames do not depend on the box")


def refused(H, call, status):
    with pytest.raises(H.VxrtError) as e:
        call()
    assert e.value.status == status


def test_refusals_change_nothing(H, scenes):
    cfg = (4, 1, 1, 1)
    with make_ctx(H, cfg) as empty:
        refused(H, empty.compact_scene, H.E_NOSCENE)
        refused(H, empty.scene_storage, H.E_NOSCENE)
        L = empty._L
        s = H.SceneStorage(7, 7, 7, 7, 7)
        assert L.vxrt_compact_scene(None) == H.E_INVALID
        assert L.vxrt_get_scene_storage(None, C.byref(s)) == H.E_INVALID and L.vxrt_get_scene_storage(empty._h, None) == H.E_INVALID
        assert s.records_live == 7 and s.leaves_capacity == 7
    pos, mrgb, size = scenes.load_scene("castle")
    with make_ctx(H, (1, 1, 1, 1), tuning=[(H.OPT_NODE_ORDER, 2)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = H.Camera(*scenes.close_camera(size))
        assert ctx.stats().node_order == 2
        before, images = ctx.read_scene(), trace_images(H, ctx, cfg, 2)
        refused(H, ctx.compact_scene, H.E_INVALID)
        assert same_arrays(ctx.read_scene(), before)
        st = ctx.scene_storage()                              # the counts are there for any scene
        assert st["records_live"] == st["records_used"] == st["records_capacity"] == len(before[0])
        for i, (a, b) in enumerate(zip(trace_images(H, ctx, cfg, 2), images)):
            assert_bits_equal(a, b, f"after the refusal: image {i}")


def test_wide_record_scenes_are_refused(H, scenes):
    require_variants(H, wide=1)
    pos, mrgb, size = scenes.load_scene("menger")
    with H.Context(W, H_, tuning=[(H.OPT_SCENE_FORMAT, 1)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        assert ctx.stats().scene_format == 1
        before = ctx.read_scene()
        refused(H, ctx.compact_scene, H.E_INVALID)
        assert same_arrays(ctx.read_scene(), before)
        assert ctx.scene_storage()["records_used"] == len(before[0])
