"""GPU: in-place scene edits and the pick query (include/vxrt_edit.h).  An edited scene must be indistinguishable from a fresh
context given the edited voxel list (tests/edit_model.py keeps that list): the decoded device tree equals the model, and every image
of every frame is bit-identical — for tracers 1 and 4, the sky cull on and off, several frames in flight and per launch."""
import ctypes as C

import numpy as np
import pytest

import edit_model as M
from conftest import assert_bits_equal, require_variants

pytestmark = pytest.mark.gpu

W, H_, BOUNCES = 96, 64, 3
TRACE_IMAGES = (0, 1, 2)            # SAMPLED_COLOR, NORMAL_DEPTH, ALBEDO_NODE
# (tracer, sky cull, frames in flight, frames per launch)
CONFIGS = [(1, 1, 1, 1), (4, 0, 1, 1), (4, 1, 2, 8), (1, 0, 2, 8)]


def make_ctx(H, cfg, tuning=()):
    tracer, cull, fif, fpl = cfg
    return H.Context(W, H_, max_bounces=BOUNCES, tracer=tracer, frames_in_flight=fif, frames_per_launch=fpl,
                     tuning=[(H.OPT_SKY_CULL, cull)] + list(tuning))


def base_scene(H, scenes, name):
    """-> (loader(ctx), model dict, camera, depth).  'startup' is the reference's start-up scene; 'menger_device' the level-3 sponge
    that vxrt_set_menger builds on the device (no host copy of its records exists)."""
    if name == "startup":
        pos, mrgb = H.default_scene_voxels(1)
        cam = scenes.reference_start_camera()
        load = lambda c: c.recreate_octree(pos, mrgb)   # noqa: E731
    elif name == "menger_device":
        mrgb0 = (0, 0xB0, 0xD0, 0x60)
        pos, mrgb = H.menger_voxels(3, mrgb0)
        cam = scenes.close_camera((27, 27, 27))
        load = lambda c: c.set_menger(3, 0, mrgb0)   # noqa: E731
    else:
        pos, mrgb, size = scenes.load_scene(name)
        cam = scenes.close_camera(size)
        load = lambda c: c.recreate_octree(pos, mrgb)   # noqa: E731
    _, depth = H.build_octree(pos, mrgb)
    return load, M.from_list(pos, mrgb), cam, depth


def fresh(H, cfg, model, cam, tuning=()):
    c = make_ctx(H, cfg, tuning)
    c.recreate_octree(*M.to_list(model))
    c.camera = H.Camera(*cam)
    return c


def trace_images(H, ctx, cfg, frame):
    ctx.set_frame_number(frame)
    if cfg[3] > 1:
        ctx.render_frames(H.TRACE, cfg[3])
    else:
        ctx.render(H.TRACE)
    return [ctx.read(i) for i in TRACE_IMAGES]


def pipeline_images(H, ctx, cfg, frame):
    ctx.reset_history()
    ctx.set_frame_number(frame)
    if cfg[3] > 1:
        ctx.render_frames(H.ALL, cfg[3])
    else:
        ctx.render(H.ALL)
        ctx.render(H.ALL)
    return [ctx.read(i) for i in (H.ACCUM_COLOR, H.DENOISED)] + [ctx.read(H.DISPLAY_RGBA8_SRGB)]


def assert_same_frames(H, edited, reference, cfg, frame, what):
    for i, (a, b) in enumerate(zip(trace_images(H, edited, cfg, frame), trace_images(H, reference, cfg, frame))):
        assert_bits_equal(a, b, f"{what}: trace image {i}")
    got, want = pipeline_images(H, edited, cfg, frame + 20), pipeline_images(H, reference, cfg, frame + 20)
    for i in range(2):
        assert_bits_equal(got[i], want[i], f"{what}: pipeline image {i}")
    assert np.array_equal(got[2], want[2]), f"{what}: display"


def batches(model, depth, seed):
    """The issue's batch kinds, seeded: new branches from the root, recolours, single and subtree clears, duplicates in a batch,
    set and clear of one voxel across calls.  Yields (label, pos, mrgb or None)."""
    rng = np.random.default_rng(seed)
    lim = 1 << depth
    keys = np.array(sorted(model), np.int64)
    colour = lambda n: rng.integers(0, 256, size=(n, 4)).astype(np.uint8)   # noqa: E731
    # an octant of the root the scene leaves empty (the .vox scenes sit in x, y, z >= 0) gets a branch of its own
    occupied = {tuple(o) for o in np.unique((keys >= 0).astype(np.int64), axis=0).tolist()}
    empty = [o for o in np.ndindex(2, 2, 2) if o not in occupied]
    octant = np.array(empty[0] if empty else (0, 0, 0))
    lo = np.where(octant == 1, 0, -lim)
    branch = (lo + rng.integers(0, lim, size=(12, 3))).astype(np.int16)
    yield "new branches", branch, colour(len(branch))
    pick = keys[rng.choice(len(keys), size=min(24, len(keys)), replace=False)]
    yield "recolour", pick.astype(np.int16), colour(len(pick))
    yield "clear single voxels", pick[:8].astype(np.int16), None
    # a whole subtree: every voxel of the aligned 4^3 cell around one voxel, and the branch built above
    cell = (keys[len(keys) // 2] // 4) * 4
    sub = np.array([cell + np.array(o) for o in np.ndindex(4, 4, 4)], np.int16)
    yield "clear subtrees", np.concatenate([sub, branch]), None
    dup = np.concatenate([pick[8:16], pick[8:16], branch[:4], branch[:4]]).astype(np.int16)
    yield "duplicates in a batch", dup, colour(len(dup))
    one = branch[5:6]
    yield "set one voxel", one, colour(1)
    yield "clear it again", one, None
    yield "and set it again", one, colour(1)


SCENES = ["menger", "castle", "startup", "menger_device"]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "tracer%d-cull%d-fif%d-fpl%d" % c)
@pytest.mark.parametrize("name", SCENES)
def test_edits_equal_a_rebuild(H, scenes, name, cfg):
    load, model, cam, depth = base_scene(H, scenes, name)
    with make_ctx(H, cfg) as ctx:
        load(ctx)
        assert ctx.stats().octree_depth == depth
        ctx.camera = H.Camera(*cam)
        anchor = np.array([[-(1 << depth)] * 3], np.int16)   # pins the depth of every model below (fresh builds included)
        ctx.edit_voxels(anchor, [[3, 40, 50, 60]])
        M.apply(model, anchor, [[3, 40, 50, 60]])
        for k, (label, pos, mrgb) in enumerate(batches(model, depth, seed=7)):
            if mrgb is None:
                ctx.clear_voxels(pos)
            else:
                ctx.edit_voxels(pos, mrgb)
            M.apply(model, pos, mrgb)
            svo, leaves = ctx.read_scene()
            assert M.decode_records(svo, leaves, depth) == model, label
            assert ctx.stats().octree_nodes == len(H.build_records(*M.to_list(model))[0]), label
            with fresh(H, cfg, model, cam) as ref:
                assert ref.stats().octree_depth == depth
                assert_same_frames(H, ctx, ref, cfg, 3 + 2 * k, f"{name} {label}")


@pytest.mark.parametrize("tracer", [2, 3, 5])
def test_edits_equal_a_rebuild_variant_tracers(H, scenes, tracer):
    require_variants(H, tracer=tracer)          # they live in libvxrt_variants.so, loaded beside the product for this test
    cfg = (tracer, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    with make_ctx(H, cfg) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        for k, (label, pos, mrgb) in enumerate(batches(model, depth, seed=11)):
            (ctx.clear_voxels(pos) if mrgb is None else ctx.edit_voxels(pos, mrgb))
            M.apply(model, pos, mrgb)
            if len(H.build_records(*M.to_list(model))[0]) and H.build_octree(*M.to_list(model))[1] == depth:
                with fresh(H, cfg, model, cam) as ref:
                    for i, (a, b) in enumerate(zip(trace_images(H, ctx, cfg, k), trace_images(H, ref, cfg, k))):
                        assert_bits_equal(a, b, f"tracer {tracer} {label} {i}")


def test_sky_cull_box_grows_with_a_far_voxel(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    with make_ctx(H, cfg) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        before = ctx.stats()
        culled_before = ctx.culled_pixels()
        assert before.cull_box_valid and culled_before > 0
        # a voxel in the camera's view and outside the old box: on the view axis, between the camera and the scene
        p, d, _ = cam
        d = np.asarray(d, np.float64) / np.linalg.norm(d)
        q = np.asarray(p, np.float64) + d * 1.0
        assert np.any(q < np.array(before.cull_box_min)) or np.any(q >= np.array(before.cull_box_max))
        far = np.floor(2 * q).astype(np.int16).reshape(1, 3)
        assert tuple(far[0]) not in model
        far_model = M.apply(dict(model), far, [[1, 250, 10, 10]])
        ctx.edit_voxels(far, [[1, 250, 10, 10]])
        after = ctx.stats()
        assert np.all(np.array(after.cull_box_min) <= np.array(before.cull_box_min))
        assert list(after.cull_box_min) != list(before.cull_box_min) or list(after.cull_box_max) != list(before.cull_box_max)
        with fresh(H, cfg, far_model, cam) as ref:
            got, want = ref.stats(), after
            assert got.octree_depth == depth
            assert list(got.cull_box_min) == list(want.cull_box_min) and list(got.cull_box_max) == list(want.cull_box_max)
            hit = ctx.pick(np.asarray(p, np.float32).reshape(1, 3), np.asarray(d, np.float32).reshape(1, 3))
            assert hit["status"][0] == 1 and list(hit["voxel"][0]) == list(far[0])
            assert_same_frames(H, ctx, ref, cfg, 5, "far voxel")


def test_storage_grows_across_reallocations_and_is_deterministic(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "castle")
    rng = np.random.default_rng(5)
    lim = 1 << depth
    contexts = [make_ctx(H, cfg), make_ctx(H, cfg)]
    sizes = []
    try:
        for c in contexts:
            load(c)
            c.camera = H.Camera(*cam)
        anchor = np.array([[-lim] * 3], np.int16)
        for c in contexts:
            c.edit_voxels(anchor, [[0, 9, 9, 9]])
        M.apply(model, anchor, [[0, 9, 9, 9]])
        for k in range(6):
            n = 500 * 4 ** k if k < 5 else 3000
            pos = rng.integers(-lim, lim, size=(n, 3)).astype(np.int16)
            mrgb = rng.integers(0, 256, size=(n, 4)).astype(np.uint8)
            clear = k == 5
            for c in contexts:
                (c.clear_voxels(pos) if clear else c.edit_voxels(pos, mrgb))
            M.apply(model, pos, None if clear else mrgb)
            sizes.append(contexts[0].stats().scene_bytes)
            a, b = contexts[0].read_scene(), contexts[1].read_scene()
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two contexts, same edits: same records"
            assert M.decode_records(*a, depth) == model
        assert len(set(sizes[:5])) >= 3, sizes        # the storage was re-allocated several times
        with fresh(H, cfg, model, cam) as ref:
            assert_same_frames(H, contexts[0], ref, cfg, 9, "after growth")
    finally:
        for c in contexts:
            c.close()


def test_edits_that_change_nothing_keep_every_frame(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    some = np.array(sorted(model)[:5], np.int16)
    words = np.array([model[tuple(p)] for p in some.tolist()], np.int64).astype(np.uint32)
    same_mrgb = np.stack([(words >> 24) & 0x7F, (words >> 16) & 0xFF, (words >> 8) & 0xFF, words & 0xFF], 1).astype(np.uint8)
    absent = np.array([[-(1 << depth) + 1] * 3], np.int16)
    assert tuple(absent[0]) not in model
    with make_ctx(H, cfg) as a, make_ctx(H, cfg) as b:
        for c in (a, b):
            load(c)
            c.camera = H.Camera(*cam)
            c.render(H.ALL)
            c.render(H.ALL)
        before = a.read_scene()
        a.edit_voxels(some, same_mrgb)
        a.clear_voxels(absent)
        a.edit_voxels(np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8))
        after = a.read_scene()
        assert M.decode_records(*after, depth) == M.decode_records(*before, depth)
        for _ in range(3):
            a.render(H.ALL)
            b.render(H.ALL)
        for i in (H.SAMPLED_COLOR, H.NORMAL_DEPTH, H.ACCUM_COLOR, H.DENOISED):
            assert_bits_equal(a.read(i), b.read(i), f"no-op edit: image {i}")


def test_frame_enqueued_before_an_edit_sees_the_old_scene(H, scenes):
    cfg = (4, 1, 2, 1)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    with make_ctx(H, cfg) as ctx, fresh(H, cfg, model, cam) as old_ref:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        ctx.set_frame_number(4)
        old_ref.set_frame_number(4)
        ctx.render(H.TRACE)                       # enqueued, not waited for
        gone = np.array([p for p in model if p[1] >= 9], np.int16)   # the top third of the sponge
        ctx.clear_voxels(gone)
        old_ref.render(H.TRACE)
        for i in TRACE_IMAGES:
            assert_bits_equal(ctx.read(i), old_ref.read(i), f"before the edit: image {i}")
        M.apply(model, gone, None)
        with fresh(H, cfg, model, cam) as new_ref:
            assert new_ref.stats().octree_depth == depth
            new_ref.set_frame_number(5)
            new_ref.render(H.TRACE)
            ctx.render(H.TRACE)
            for i in TRACE_IMAGES:
                assert_bits_equal(ctx.read(i), new_ref.read(i), f"after the edit: image {i}")


def test_refusals_change_nothing(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "menger")
    L = H.lib()
    with make_ctx(H, cfg) as empty:
        with pytest.raises(H.VxrtError) as e:
            empty.edit_voxels([[0, 0, 0]], [[1, 2, 3, 4]])
        assert e.value.status == H.E_NOSCENE
        with pytest.raises(H.VxrtError) as e:
            empty.pick([[0, 0, -5]], [[0, 0, 1]])
        assert e.value.status == H.E_NOSCENE
    with make_ctx(H, cfg) as ctx, make_ctx(H, cfg) as ref:
        for c in (ctx, ref):
            load(c)
            c.camera = H.Camera(*cam)
        before = ctx.read_scene()
        lim = 1 << depth
        outside = np.array([[0, 0, 0], [lim, 0, 0]], np.int16)       # one inside, one outside: all or nothing
        with pytest.raises(H.VxrtError) as e:
            ctx.edit_voxels(outside, [[1, 1, 1, 1]] * 2)
        assert e.value.status == H.E_SCENE
        with pytest.raises(H.VxrtError) as e:
            ctx.clear_voxels([[1, 1, 1], [0, -lim - 1, 0]])
        assert e.value.status == H.E_SCENE
        assert ctx._L.vxrt_edit_voxels(ctx._h, None, None, C.c_size_t(3)) == H.E_INVALID
        after = ctx.read_scene()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        for i, (a, b) in enumerate(zip(trace_images(H, ctx, cfg, 2), trace_images(H, ref, cfg, 2))):
            assert_bits_equal(a, b, f"after refusals: image {i}")
    assert L.vxrt_edit_voxels(None, None, None, C.c_size_t(0)) == H.E_INVALID


def test_treelet_scenes_are_refused(H, scenes):
    pos, mrgb, size = scenes.load_scene("castle")
    with make_ctx(H, (1, 1, 1, 1), tuning=[(H.OPT_NODE_ORDER, 2)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        assert ctx.stats().node_order == 2
        before = ctx.read_scene()
        with pytest.raises(H.VxrtError) as e:
            ctx.edit_voxels(pos[:1], [[1, 2, 3, 4]])
        assert e.value.status == H.E_INVALID
        after = ctx.read_scene()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_wide_record_scenes_are_refused(H, scenes):
    require_variants(H, wide=1)
    pos, mrgb, size = scenes.load_scene("menger")
    with H.Context(W, H_, tuning=[(H.OPT_SCENE_FORMAT, 1)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        assert ctx.stats().scene_format == 1
        with pytest.raises(H.VxrtError) as e:
            ctx.edit_voxels(pos[:1], [[1, 2, 3, 4]])
        assert e.value.status == H.E_INVALID


def test_two_ranks_apply_the_same_edits(H, scenes):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = base_scene(H, scenes, "castle")
    rng = np.random.default_rng(2)
    keys = np.array(sorted(model), np.int16)
    pos = keys[rng.choice(len(keys), 200, replace=False)]
    mrgb = rng.integers(0, 256, size=(200, 4)).astype(np.uint8)
    with make_ctx(H, cfg) as single:
        ranks = [H.Context(W, H_, max_bounces=BOUNCES, tracer=4, rank=r, nranks=2, band_rows=16) for r in range(2)]
        try:
            for c in [single] + ranks:
                load(c)
                c.camera = H.Camera(*cam)
                c.edit_voxels(pos, mrgb)
                c.clear_voxels(pos[:50])
                c.set_frame_number(6)
                c.render(H.TRACE)
            full = single.read(H.SAMPLED_COLOR)
            for c in ranks:
                rows = c.local_rows()
                assert_bits_equal(c.read(H.SAMPLED_COLOR), full[rows], "rank rows")
        finally:
            for c in ranks:
                c.close()


def slab_entry(o, d, voxel):
    """binary64 entry / exit of the ray into voxel `voxel`'s world cube [v/2, v/2 + 1/2)^3."""
    lo = np.asarray(voxel, np.float64) * 0.5
    hi = lo + 0.5
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    near, far = np.minimum(t0, t1), np.maximum(t0, t1)
    return np.nanmax(near), np.nanmin(far)


def check_picks(H, ctx, model, origins, dirs):
    got = ctx.pick(origins, dirs)
    hit, time, node, normal = ctx.cast_rays(origins, dirs)
    assert np.array_equal(got["status"] != 0, hit)
    assert np.array_equal(got["time"].view(np.uint32), time.view(np.uint32))
    assert np.array_equal(got["leaf"], node)
    assert np.array_equal(got["normal"].view(np.uint32), normal.view(np.uint32))
    hits = np.flatnonzero(got["status"] == 1)
    for i in hits:
        v = tuple(int(x) for x in got["voxel"][i])
        assert model.get(v) == int(got["leaf"][i]), (i, v)
        entry, exit_ = slab_entry(origins[i].astype(np.float64), dirs[i].astype(np.float64), v)
        t = float(got["time"][i])
        assert abs(max(entry, 0.0) - t) <= 1e-5 * max(1.0, t) and t <= exit_ + 1e-5 * max(1.0, t), (i, v, entry, exit_, t)
    return got


@pytest.mark.parametrize("name", ["menger", "castle", "menger_device"])
def test_pick_equals_the_walk_and_finds_the_voxel(H, scenes, name):
    load, model, cam, depth = base_scene(H, scenes, name)
    rng = np.random.default_rng(4)
    with make_ctx(H, (4, 1, 1, 1)) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        xs, ys = np.meshgrid(np.arange(0, W, 3), np.arange(0, H_, 3))
        o, d = ctx.pixel_rays(xs.ravel(), ys.ravel())
        got = check_picks(H, ctx, model, o, d)
        assert (got["status"] == 1).sum() > len(o) // 4
        pp = ctx.pick_pixels(xs.ravel(), ys.ravel())
        for k in got:
            assert np.array_equal(pp[k], got[k]), k
        # random rays from around the scene, some starting inside it
        centre = np.mean(np.array(sorted(model), np.float64), 0) * 0.5
        ro = (centre + rng.normal(0, 12, size=(2000, 3))).astype(np.float32)
        rd = rng.normal(size=(2000, 3)).astype(np.float32)
        rd[:20, 0] = 0.0            # direction components that are exactly 0: the shader's own walk
        check_picks(H, ctx, model, ro, rd)
        # picks see edits: break what the camera rays hit, and place a voxel on the face they hit
        one_face = np.count_nonzero(got["normal"], axis=1) == 1      # a face, not an edge or a corner
        first = np.flatnonzero((got["status"] == 1) & one_face)[:40]
        voxels = got["voxel"][first]
        placed = voxels + got["normal"][first].astype(np.int32)
        lim = 1 << depth
        inside = np.all((placed >= -lim) & (placed < lim), axis=1)
        ctx.edit_voxels(placed[inside].astype(np.int16), [[2, 200, 100, 50]] * int(inside.sum()))
        M.apply(model, placed[inside].astype(np.int16), [[2, 200, 100, 50]] * int(inside.sum()))
        again = check_picks(H, ctx, model, o[first], d[first])
        # each ray now stops at a placed voxel (its own, or a neighbour's placed in front of it), no later than before
        placed_set = {tuple(v) for v in placed[inside].tolist()}
        assert np.all(again["status"][inside] == 1)
        assert all(tuple(v) in placed_set for v in again["voxel"][inside].tolist())
        assert np.all(again["time"][inside] <= got["time"][first][inside])
        ctx.clear_voxels(placed[inside].astype(np.int16))
        ctx.clear_voxels(voxels.astype(np.int16))
        M.apply(model, placed[inside].astype(np.int16), None)
        M.apply(model, voxels.astype(np.int16), None)
        third = check_picks(H, ctx, model, o[first], d[first])
        hit3 = third["status"] == 1
        assert not any(tuple(v) in {tuple(x) for x in voxels.tolist()} for v in third["voxel"][hit3].tolist())
