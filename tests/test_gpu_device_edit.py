"""GPU: editing and reading a loaded scene through voxel lists in device memory (include/vxrt_device_edit.h).  Every case runs a
context given device lists beside a twin given the same lists through edit_voxels / clear_voxels, and every comparison is bit for
bit: the records and leaf words in use, the stats with the sky-cull box, the read-back, every image of every frame with the temporal
history kept.  get_voxels_device equals get_voxels in count, order, positions and bytes.  Refused calls change nothing."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import edit_model as M
from conftest import assert_bits_equal, require_variants
from test_gpu_device_build import assert_same_scene
from test_gpu_edit import CONFIGS, H_, W, assert_same_frames, batches, make_ctx, trace_images

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
MRGB0 = (0, 0xB0, 0xD0, 0x60)
CFG = (4, 1, 1, 1)
SCENES = ["menger", "castle", "startup", "device_sponge", "empty", "depth0", "depth1", "depth2", "depth3"]


def scene(H, scenes, name):
    """-> (loader(ctx), model dict, camera)"""
    if name in ("menger", "castle"):
        pos, mrgb, size = scenes.load_scene(name)
        return (lambda c: c.recreate_octree(pos, mrgb)), M.from_list(pos, mrgb), scenes.close_camera(size)
    if name == "startup":
        pos, mrgb = H.default_scene_voxels(1)
        return (lambda c: c.recreate_octree(pos, mrgb)), M.from_list(pos, mrgb), scenes.reference_start_camera()
    if name == "device_sponge":
        pos, mrgb = H.menger_voxels(3, MRGB0)
        return (lambda c: c.set_voxels_device(pos, mrgb)), M.from_list(pos, mrgb), scenes.close_camera((27, 27, 27))
    if name == "empty":
        pos, mrgb = np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    else:
        depth = int(name[-1])
        rng = np.random.default_rng(40 + depth)
        lim = 1 << depth
        # both far corners pin the depth
        pos = np.concatenate([rng.integers(-lim, lim, (3 * lim * lim, 3)), [[-lim] * 3, [lim - 1] * 3]]).astype(np.int16)
        mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    return (lambda c: c.recreate_octree(pos, mrgb)), M.from_list(pos, mrgb), scenes.close_camera((4, 4, 4))


def twins(H, load, cam, cfg=CFG, tuning=()):
    """-> (the context that gets device lists, its twin that gets host lists), both loaded"""
    dev, host = make_ctx(H, cfg, tuning), make_ctx(H, cfg, tuning)
    for c in (dev, host):
        load(c)
        c.camera = H.Camera(*cam)
    return dev, host


def on_device(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def apply_both(dev, host, pos, mrgb):
    """One batch: device tensors to `dev`, the same arrays through the host call to `host`."""
    pos = np.ascontiguousarray(pos, np.int16).reshape(-1, 3)
    if mrgb is None:
        dev.clear_voxels_device(on_device(pos))
        host.clear_voxels(pos)
    else:
        mrgb = np.ascontiguousarray(mrgb, np.uint8).reshape(-1, 4)
        dev.edit_voxels_device(on_device(pos), on_device(mrgb))
        host.edit_voxels(pos, mrgb)


def assert_same_state(dev, host, what):
    assert_same_scene(dev, host, what)                      # read_scene() over the counts in use, stats(), the cull box
    assert dev.stats().octree_nodes == host.stats().octree_nodes, what
    for a, b in zip(dev.get_voxels(), host.get_voxels()):
        assert np.array_equal(a, b), f"{what}: get_voxels"


def history_images(H, ctx, cfg):
    """Two more frames of the whole pipeline on top of the history the context has."""
    if cfg[3] > 1:
        ctx.render_frames(H.ALL, cfg[3])
    else:
        ctx.render(H.ALL)
        ctx.render(H.ALL)
    return [ctx.read(i) for i in (H.ACCUM_COLOR, H.DENOISED)] + [ctx.read(H.DISPLAY_RGBA8_SRGB)]


def assert_same_history(H, dev, host, cfg, what):
    got, want = history_images(H, dev, cfg), history_images(H, host, cfg)
    for i in range(2):
        assert_bits_equal(got[i], want[i], f"{what}: image {i} with the history kept")
    assert np.array_equal(got[2], want[2]), f"{what}: display with the history kept"


def cube_batches(model, depth, seed):
    """test_gpu_edit's batch sequence, with the positions that fall outside the root cube dropped (its 4^3 subtree clear leaves the
    cube of a depth 0 or 1 scene; a list with one position outside is refused as a whole, which the refusal test covers)."""
    lim = 1 << depth
    for label, pos, mrgb in batches(model, depth, seed):
        pos = np.asarray(pos).reshape(-1, 3)
        keep = np.all((pos >= -lim) & (pos < lim), axis=1)
        yield label, pos[keep], (None if mrgb is None else np.asarray(mrgb)[keep])


# ---- equal to the host call ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENES)
def test_device_lists_equal_the_host_call(H, scenes, name):
    load, model0, cam = scene(H, scenes, name)
    for cfg in CONFIGS:
        model = dict(model0)
        dev, host = twins(H, load, cam, cfg)
        with dev, host:
            depth = dev.scene_depth
            assert depth == host.scene_depth
            for c in (dev, host):                      # a temporal history before the first edit
                c.set_frame_number(1)
                c.render(H.ALL)
            if not model:                              # the empty scene: its first voxels, then the sequence over them
                first = np.array(list(np.ndindex(2, 2, 2)), np.int16)[:5] - (1 << depth)
                apply_both(dev, host, first, [[1, 10, 20, 30]] * len(first))
                M.apply(model, first, [[1, 10, 20, 30]] * len(first))
                assert_same_state(dev, host, f"{name} {cfg}: first voxels")
            for label, pos, mrgb in cube_batches(model, depth, seed=7):
                apply_both(dev, host, pos, mrgb)
                M.apply(model, pos, mrgb)
                assert_same_state(dev, host, f"{name} {cfg}: {label}")
                if cfg == CONFIGS[0]:
                    assert M.decode_records(*dev.read_scene(), depth) == model, label
            gone = np.array(sorted(model), np.int16)   # clears that prune to the root, and clears of positions then absent
            assert_same_history(H, dev, host, cfg, f"{name} {cfg}")
            assert_same_frames(H, dev, host, cfg, 5, f"{name} {cfg}")
            apply_both(dev, host, gone, None)
            assert_same_state(dev, host, f"{name} {cfg}: everything cleared")
            assert dev.count_voxels() == 0
            apply_both(dev, host, gone[: 1 + len(gone) // 2], None)
            assert_same_state(dev, host, f"{name} {cfg}: absent positions cleared")
            assert_same_frames(H, dev, host, cfg, 9, f"{name} {cfg}: emptied")
            back = gone[::3]
            colours = np.random.default_rng(3).integers(0, 256, (len(back), 4)).astype(np.uint8)
            apply_both(dev, host, back, colours)
            assert_same_state(dev, host, f"{name} {cfg}: set again")
            assert_same_frames(H, dev, host, cfg, 11, f"{name} {cfg}: set again")


# ---- duplicates, large batches, storage growth -----------------------------------------------------------------------------------
@pytest.mark.parametrize("reverse", [False, True], ids=["given", "reversed"])
def test_the_last_entry_for_a_position_wins(H, scenes, reverse):
    load, model, cam = scene(H, scenes, "castle")
    rng = np.random.default_rng(21)
    dev, host = twins(H, load, cam)
    with dev, host:
        lim = 1 << dev.scene_depth
        distinct = rng.integers(-lim, lim, (700, 3)).astype(np.int16)
        pos = distinct[rng.integers(0, len(distinct), 60000)]          # some 85 entries per position
        mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
        if reverse:
            pos, mrgb = pos[::-1].copy(), mrgb[::-1].copy()
        apply_both(dev, host, pos, mrgb)
        M.apply(model, pos, mrgb)
        assert_same_state(dev, host, "duplicates")
        assert M.from_list(*dev.get_voxels()) == model
        some = distinct[rng.integers(0, len(distinct), 9000)]
        apply_both(dev, host, some, None)                              # a clear list with duplicates
        M.apply(model, some, None)
        assert_same_state(dev, host, "duplicate clears")
        assert M.from_list(*dev.get_voxels()) == model
        assert_same_frames(H, dev, host, CFG, 4, "duplicates")


def test_a_batch_of_2_20_entries_on_the_device_sponge(H, scenes):
    load, model, cam = scene(H, scenes, "device_sponge")
    rng = np.random.default_rng(22)
    dev, host = twins(H, load, cam)
    with dev, host:
        lim = 1 << dev.scene_depth
        n = 1 << 20
        pos = rng.integers(-lim, lim, (n, 3)).astype(np.int16)          # the cube has (2 lim)^3 = 2^18 cells: every one several times
        mrgb = rng.integers(0, 256, (n, 4)).astype(np.uint8)
        bytes_before = dev.stats().scene_bytes
        apply_both(dev, host, pos, mrgb)
        assert dev.stats().scene_bytes > bytes_before                   # the batch crossed a storage reallocation
        assert_same_state(dev, host, "2^20 sets")
        last = {}
        for i, p in enumerate(map(tuple, pos.tolist())):
            last[p] = i
        model.update({p: M.word(mrgb[i]) for p, i in last.items()})
        assert M.from_list(*dev.get_voxels()) == model
        apply_both(dev, host, pos[: n // 2], None)
        assert_same_state(dev, host, "2^19 clears")
        assert_same_frames(H, dev, host, CFG, 6, "2^20 entries")


def test_storage_grows_across_reallocations_like_the_host_calls(H, scenes):
    load, model, cam = scene(H, scenes, "castle")
    rng = np.random.default_rng(5)
    dev, host = twins(H, load, cam)
    sizes = []
    with dev, host:
        lim = 1 << dev.scene_depth
        for k in range(6):
            n = 500 * 4 ** k if k < 5 else 3000
            pos = rng.integers(-lim, lim, (n, 3)).astype(np.int16)
            mrgb = rng.integers(0, 256, (n, 4)).astype(np.uint8)
            apply_both(dev, host, pos, None if k == 5 else mrgb)
            sizes.append(dev.stats().scene_bytes)
            assert_same_state(dev, host, f"growth step {k}")
        assert len(set(sizes[:5])) >= 3, sizes                          # the storage was re-allocated several times
        assert_same_frames(H, dev, host, CFG, 9, "after growth")


def test_two_contexts_given_the_same_lists_hold_the_same_bytes(H, scenes):
    load, model, cam = scene(H, scenes, "menger")
    rng = np.random.default_rng(23)
    a, b = twins(H, load, cam)
    with a, b:
        lim = 1 << a.scene_depth
        for k in range(4):
            pos = on_device(rng.integers(-lim, lim, (20000, 3)).astype(np.int16))
            mrgb = on_device(rng.integers(0, 256, (20000, 4)).astype(np.uint8))
            for c in (a, b):
                (c.clear_voxels_device(pos) if k == 2 else c.edit_voxels_device(pos, mrgb))
            # read_scene() is every record and leaf word up to the counts in use: the unused entries of the 8-entry blocks included
            assert_same_scene(a, b, f"step {k}")
        a.edit_voxels_device(pos, mrgb)                                  # the same list twice: nothing changes the second time
        before = a.read_scene()
        a.edit_voxels_device(pos, mrgb)
        after = a.read_scene()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---- alignment ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 4099, 10007])
def test_lists_at_odd_offsets_take_both_load_paths(H, scenes, n):
    load, model, cam = scene(H, scenes, "menger")
    rng = np.random.default_rng(n)
    dev, host = twins(H, load, cam)
    with dev, host:
        lim = 1 << dev.scene_depth
        for pos_off, mrgb_off in ((0, 0), (8, 16), (1, 4), (3, 1), (8, 1), (5, 16)):   # in int16 elements / in bytes
            pos = rng.integers(-lim, lim, (n, 3)).astype(np.int16)
            mrgb = rng.integers(0, 256, (n, 4)).astype(np.uint8)
            flat_p = torch.zeros(3 * n + 64, dtype=torch.int16, device=DEV)
            flat_m = torch.zeros(4 * n + 64, dtype=torch.uint8, device=DEV)
            tp = flat_p[pos_off: pos_off + 3 * n].view(n, 3)
            tm = flat_m[mrgb_off: mrgb_off + 4 * n].view(n, 4)
            tp.copy_(on_device(pos))
            tm.copy_(on_device(mrgb))
            assert tp.data_ptr() == flat_p.data_ptr() + 2 * pos_off and tm.data_ptr() == flat_m.data_ptr() + mrgb_off
            assert flat_p.data_ptr() % 16 == 0 and flat_m.data_ptr() % 16 == 0
            dev.edit_voxels_device(tp, tm)
            host.edit_voxels(pos, mrgb)
            assert_same_state(dev, host, f"n {n}, offsets {pos_off} / {mrgb_off}: set")
            dev.clear_voxels_device(tp[: n // 2 + 1])
            host.clear_voxels(pos[: n // 2 + 1])
            assert_same_state(dev, host, f"n {n}, offsets {pos_off} / {mrgb_off}: clear")


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def snapshot(H, ctx, frame):
    svo, leaves = ctx.read_scene()
    t = ctx.stats()
    stats = (t.octree_depth, t.octree_nodes, t.scene_bytes, t.cull_box_valid, list(t.cull_box_min), list(t.cull_box_max))
    return svo, leaves, stats, trace_images(H, ctx, CFG, frame)


def assert_unchanged(H, ctx, before, frame, what):
    svo, leaves, stats, images = snapshot(H, ctx, frame)
    assert np.array_equal(svo, before[0]) and np.array_equal(leaves, before[1]), f"{what}: scene bytes"
    assert stats == before[2], f"{what}: stats"
    for i, (a, b) in enumerate(zip(images, before[3])):
        assert_bits_equal(a, b, f"{what}: image {i}")


def test_refusals_change_nothing(H, scenes):
    load, model, cam = scene(H, scenes, "menger")
    rng = np.random.default_rng(31)
    hip = C.CDLL("libamdhip64.so")
    with make_ctx(H, CFG) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        L = ctx._L
        lim = 1 << ctx.scene_depth
        before = snapshot(H, ctx, 3)
        n = 300000
        pos = rng.integers(-lim, lim, (n, 3)).astype(np.int16)
        mrgb = on_device(rng.integers(0, 256, (n, 4)).astype(np.uint8))
        ptr = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
        # one position a cell outside the cube, in the middle of a large valid list
        for k, bad in enumerate(([lim, 0, 0], [0, -lim - 1, 0], [1, 2, lim])):
            p = pos.copy()
            p[n // 2 + k] = bad
            with pytest.raises(H.VxrtError) as e:
                ctx.edit_voxels_device(on_device(p), mrgb)
            assert e.value.status == H.E_SCENE and "root cube" in str(e.value)
            with pytest.raises(H.VxrtError) as e:
                ctx.clear_voxels_device(on_device(p))
            assert e.value.status == H.E_SCENE
            assert_unchanged(H, ctx, before, 3, f"outside {bad}")
        good = on_device(pos)
        torch.cuda.synchronize()
        # pinned host memory
        pin_p, pin_m = torch.as_tensor(pos).pin_memory(), mrgb.cpu().pin_memory()
        assert L.vxrt_edit_voxels_device(ctx._h, ptr(pin_p), ptr(pin_m), C.c_size_t(n)) == H.E_INVALID
        assert L.vxrt_edit_voxels_device(ctx._h, ptr(pin_p), None, C.c_size_t(n)) == H.E_INVALID
        assert L.vxrt_edit_voxels_device(ctx._h, ptr(good), ptr(pin_m), C.c_size_t(n)) == H.E_INVALID
        assert L.vxrt_edit_voxels_device(ctx._h, pos.ctypes.data_as(C.c_void_p), None, C.c_size_t(n)) == H.E_INVALID    # pageable
        assert_unchanged(H, ctx, before, 3, "host pointers")
        # an n that runs past the allocation (allocations of their own: their extent is exact)
        raw_p, raw_m = C.c_void_p(), C.c_void_p()
        assert hip.hipMalloc(C.byref(raw_p), C.c_size_t(64 * 6)) == 0 and hip.hipMalloc(C.byref(raw_m), C.c_size_t(64 * 4)) == 0
        assert hip.hipMemset(raw_p, 0, C.c_size_t(64 * 6)) == 0 and hip.hipMemset(raw_m, 0, C.c_size_t(64 * 4)) == 0
        assert hip.hipDeviceSynchronize() == 0
        assert L.vxrt_edit_voxels_device(ctx._h, raw_p, raw_m, C.c_size_t(65)) == H.E_INVALID
        assert L.vxrt_edit_voxels_device(ctx._h, raw_p, None, C.c_size_t(65)) == H.E_INVALID
        assert L.vxrt_edit_voxels_device(ctx._h, ptr(good), raw_m, C.c_size_t(65)) == H.E_INVALID
        assert L.vxrt_edit_voxels_device(ctx._h, raw_p, raw_m, C.c_size_t(1 << 32)) == H.E_INVALID
        assert_unchanged(H, ctx, before, 3, "past the allocation")
        # a null pos with n > 0
        assert L.vxrt_edit_voxels_device(ctx._h, None, ptr(mrgb), C.c_size_t(n)) == H.E_INVALID
        assert L.vxrt_edit_voxels_device(ctx._h, None, None, C.c_size_t(1)) == H.E_INVALID
        assert_unchanged(H, ctx, before, 3, "null pos")
        # n == 0 does nothing, whatever the pointers
        assert L.vxrt_edit_voxels_device(ctx._h, None, None, C.c_size_t(0)) == 0
        ctx.edit_voxels_device(np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8))
        ctx.clear_voxels_device(torch.zeros((0, 3), dtype=torch.int16, device=DEV))
        assert_unchanged(H, ctx, before, 3, "n == 0")
        # get_voxels_device refusals: host memory, past the allocation, one array without the other
        cnt = C.c_size_t(0)
        count = ctx.count_voxels()
        assert count > 64
        assert L.vxrt_get_voxels_device(ctx._h, None, None, ptr(pin_p), ptr(pin_m), C.c_size_t(n), C.byref(cnt)) == H.E_INVALID
        assert L.vxrt_get_voxels_device(ctx._h, None, None, raw_p, raw_m, C.c_size_t(count), C.byref(cnt)) == H.E_INVALID
        assert L.vxrt_get_voxels_device(ctx._h, None, None, ptr(good), None, C.c_size_t(n), C.byref(cnt)) == H.E_INVALID
        assert L.vxrt_get_voxels_device(ctx._h, None, None, ptr(good), ptr(mrgb), C.c_size_t(n), None) == H.E_INVALID
        assert_unchanged(H, ctx, before, 3, "get_voxels_device refusals")
        # ... and the valid list is accepted afterwards
        assert L.vxrt_edit_voxels_device(ctx._h, raw_p, raw_m, C.c_size_t(64)) == 0
        assert hip.hipFree(raw_p) == 0 and hip.hipFree(raw_m) == 0
    with make_ctx(H, CFG) as none:                                               # no scene loaded
        one_p, one_m = torch.zeros((1, 3), dtype=torch.int16, device=DEV), torch.zeros((1, 4), dtype=torch.uint8, device=DEV)
        with pytest.raises(H.VxrtError) as e:
            none.edit_voxels_device(one_p, one_m)
        assert e.value.status == H.E_NOSCENE
        with pytest.raises(H.VxrtError) as e:
            none.clear_voxels_device(one_p)
        assert e.value.status == H.E_NOSCENE
        with pytest.raises(H.VxrtError) as e:
            none.get_voxels_device()
        assert e.value.status == H.E_NOSCENE


def test_treelet_scenes_are_refused_and_read(H, scenes):
    pos, mrgb, size = scenes.load_scene("castle")
    with make_ctx(H, (1, 1, 1, 1), tuning=[(H.OPT_NODE_ORDER, 2)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = H.Camera(*scenes.close_camera(size))
        assert ctx.stats().node_order == 2
        before = ctx.read_scene()
        for call in (lambda: ctx.edit_voxels_device(on_device(pos[:1]), on_device(mrgb[:1])), lambda: ctx.clear_voxels_device(on_device(pos[:1]))):
            with pytest.raises(H.VxrtError) as e:
                call()
            assert e.value.status == H.E_INVALID
        after = ctx.read_scene()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert_get_equal(ctx, None, None, "treelet order")
        assert_get_equal(ctx, (1, 2, 3), (9, 14, 11), "treelet order, a box")


def test_wide_record_scenes_are_refused_and_read(H, scenes):
    require_variants(H, wide=1)
    pos, mrgb, size = scenes.load_scene("menger")
    with H.Context(W, H_, tuning=[(H.OPT_SCENE_FORMAT, 1)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        assert ctx.stats().scene_format == 1
        before = ctx.read_scene()
        for call in (lambda: ctx.edit_voxels_device(on_device(pos[:1]), on_device(mrgb[:1])), lambda: ctx.clear_voxels_device(on_device(pos[:1]))):
            with pytest.raises(H.VxrtError) as e:
                call()
            assert e.value.status == H.E_INVALID
        after = ctx.read_scene()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        assert_get_equal(ctx, None, None, "wide records")
        assert_get_equal(ctx, (1, 2, 3), (9, 14, 11), "wide records, a box")


# ---- ordering ----------------------------------------------------------------------------------------------------------------------
def test_a_list_written_on_a_side_stream_is_read_whole(H, scenes):
    load, model, cam = scene(H, scenes, "castle")
    rng = np.random.default_rng(33)
    dev, host = twins(H, load, cam)
    with dev, host:
        lim = 1 << dev.scene_depth
        pos = rng.integers(-lim, lim, (400000, 3)).astype(np.int16)
        mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
        src_p, src_m = on_device(pos), on_device(mrgb)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(DEV)
        with torch.cuda.stream(side):
            tp, tm = torch.zeros_like(src_p), torch.zeros_like(src_m)
            torch.cuda._sleep(50_000_000)               # the producer is still busy when the edit is asked for
            tp.copy_(src_p)
            tm.copy_(src_m)
            dev.edit_voxels_device(tp, tm)
        host.edit_voxels(pos, mrgb)
        assert_same_state(dev, host, "side stream")


def test_a_frame_enqueued_before_a_device_edit_sees_the_old_scene(H, scenes):
    cfg = (4, 1, 2, 1)
    load, model, cam = scene(H, scenes, "menger")
    with make_ctx(H, cfg) as ctx, make_ctx(H, cfg) as old_ref, make_ctx(H, cfg) as new_ref:
        for c in (ctx, old_ref, new_ref):
            load(c)
            c.camera = H.Camera(*cam)
        gone = np.array([p for p in model if p[1] >= 9], np.int16)   # the top third of the sponge
        new_ref.clear_voxels(gone)
        gone_dev = on_device(gone)
        torch.cuda.synchronize()
        ctx.set_frame_number(4)
        old_ref.set_frame_number(4)
        ctx.render(H.TRACE)                           # enqueued, not waited for
        ctx.clear_voxels_device(gone_dev)
        old_ref.render(H.TRACE)
        for i in (0, 1, 2):
            assert_bits_equal(ctx.read(i), old_ref.read(i), f"before the edit: image {i}")
        new_ref.set_frame_number(5)
        new_ref.render(H.TRACE)
        ctx.render(H.TRACE)
        for i in (0, 1, 2):
            assert_bits_equal(ctx.read(i), new_ref.read(i), f"after the edit: image {i}")


# ---- after other edits -------------------------------------------------------------------------------------------------------------
def test_device_edits_after_host_edits_a_grid_edit_and_a_grow(H, scenes):
    load, model, cam = scene(H, scenes, "castle")
    rng = np.random.default_rng(34)
    dev, host = twins(H, load, cam)
    with dev, host:
        depth = dev.scene_depth
        lim = 1 << depth
        pos = rng.integers(-lim, lim, (3000, 3)).astype(np.int16)
        mrgb = rng.integers(0, 256, (3000, 4)).astype(np.uint8)
        grid = (rng.integers(0, 1 << 31, (20, 9, 13)) | np.where(rng.random((20, 9, 13)) < 0.5, 1 << 31, 0)).astype(np.uint32).view(np.int32)
        for c in (dev, host):
            c.edit_voxels(pos, mrgb)
            c.clear_voxels(pos[::5])
            c.edit_voxel_grid(on_device(grid), (-7, 3, -lim), mode="replace")
            c.set_scene_depth(depth + 2)
        assert_same_state(dev, host, "before the device edits")
        lim = 1 << (depth + 2)
        for k in range(3):
            p = rng.integers(-lim, lim, (5000, 3)).astype(np.int16)
            m = rng.integers(0, 256, (5000, 4)).astype(np.uint8)
            apply_both(dev, host, p, None if k == 1 else m)
            assert_same_state(dev, host, f"device edit {k} after the others")
        assert_same_frames(H, dev, host, CFG, 7, "after other edits")


def test_grow_past_the_root_cube_then_fit_equals_a_rebuild(H, scenes):
    load, model, cam = scene(H, scenes, "menger")
    dev, host = twins(H, load, cam)
    with dev, host:
        depth = dev.scene_depth
        lim = 1 << depth
        far = np.array([[4 * lim, 1, 2], [3, -2 * lim - 1, -lim], [0, 0, 0]], np.int16)
        colours = np.array([[1, 200, 30, 40], [0, 10, 220, 30], [2, 9, 9, 9]], np.uint8)
        with pytest.raises(H.VxrtError) as e:
            dev.edit_voxels_device(on_device(far), on_device(colours))               # without grow: outside the cube
        assert e.value.status == H.E_SCENE
        dev.edit_voxels_device(on_device(far), on_device(colours), grow=True)
        host.edit_voxels(far, colours, grow=True)
        M.apply(model, far, colours)
        assert dev.scene_depth == host.scene_depth == depth + 3
        assert_same_state(dev, host, "grown")
        assert dev.fit_scene_depth() == host.fit_scene_depth() == H.scene_depth_for(M.to_list(model)[0])
        assert_same_state(dev, host, "fitted")
        with make_ctx(H, CFG) as rebuilt:
            rebuilt.recreate_octree(*M.to_list(model))
            rebuilt.camera = H.Camera(*cam)
            assert rebuilt.scene_depth == dev.scene_depth
            assert_same_frames(H, dev, rebuilt, CFG, 5, "grown and fitted against a rebuild")
        dev.clear_voxels_device(on_device(far[:2]))
        host.clear_voxels(far[:2])
        assert dev.fit_scene_depth() == host.fit_scene_depth() == depth
        assert_same_state(dev, host, "cleared and fitted back")


# ---- get_voxels_device -------------------------------------------------------------------------------------------------------------
def assert_get_equal(ctx, lo, hi, what):
    want_p, want_m = ctx.get_voxels(lo, hi)
    before = ctx.read_scene()
    got_p, got_m = ctx.get_voxels_device(lo, hi)
    assert got_p.device == DEV and got_m.device == DEV and got_p.dtype == torch.int16 and got_m.dtype == torch.uint8
    assert tuple(got_p.shape) == (len(want_p), 3) and tuple(got_m.shape) == (len(want_p), 4), what
    assert np.array_equal(got_p.cpu().numpy(), want_p), f"{what}: positions"
    assert np.array_equal(got_m.cpu().numpy(), want_m), f"{what}: mrgb"
    after = ctx.read_scene()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), f"{what}: the scene"
    return len(want_p)


@pytest.mark.parametrize("name", ["menger", "castle", "startup", "device_sponge", "empty", "depth0"])
def test_get_voxels_device_equals_get_voxels(H, scenes, name):
    load, model, cam = scene(H, scenes, name)
    rng = np.random.default_rng(35)
    with make_ctx(H, CFG) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        lim = 1 << ctx.scene_depth
        boxes = [(None, None),
                 ((-lim,) * 3, (lim,) * 3),
                 ((0, 0, 0), (16, 16, 16)),                                  # aligned
                 ((1, 3, 2), (14, 9, 17)),                                   # unaligned
                 ((3, 4, 5), (4, 5, 6)),                                     # one cell
                 ((-lim - 5, -3, 2), (4, lim + 9, 11)),                      # straddling the cube's faces
                 ((5, 5, 5), (5, 9, 9)),                                     # empty
                 ((9, 9, 9), (3, 3, 3)),
                 ((lim, 0, 0), (lim + 8, 8, 8)),                             # outside the cube
                 ((-4 * lim, -4 * lim, -4 * lim), (-2 * lim, -2 * lim, -2 * lim))]
        counts = [assert_get_equal(ctx, lo, hi, f"{name} {lo} {hi}") for lo, hi in boxes]
        assert counts[0] == counts[1] == len(model)
        assert counts[6] == counts[7] == counts[8] == counts[9] == 0
        if not model:
            return
        # after edits
        pos = rng.integers(-lim, lim, (2000, 3)).astype(np.int16)
        ctx.edit_voxels_device(on_device(pos), on_device(rng.integers(0, 256, (2000, 4)).astype(np.uint8)))
        ctx.clear_voxels_device(on_device(np.array(sorted(model), np.int16)[::3]))
        for lo, hi in boxes[:6]:
            assert_get_equal(ctx, lo, hi, f"{name} edited {lo} {hi}")
        frame = trace_images(H, ctx, CFG, 3)
        ctx.get_voxels_device()
        for i, (a, b) in enumerate(zip(trace_images(H, ctx, CFG, 3), frame)):
            assert_bits_equal(a, b, f"a read-back changes no image: {i}")


def test_get_voxels_device_counts_and_refuses_too_little_room(H, scenes):
    load, model, cam = scene(H, scenes, "castle")
    with make_ctx(H, CFG) as ctx:
        load(ctx)
        L = ctx._L
        want_p, want_m = ctx.get_voxels()
        total = len(want_p)
        lo, hi = (C.c_int32 * 3)(2, 0, 1), (C.c_int32 * 3)(12, 9, 14)
        in_box = ctx.count_voxels((2, 0, 1), (12, 9, 14))
        assert 0 < in_box < total
        n = C.c_size_t(0)
        assert L.vxrt_get_voxels_device(ctx._h, None, None, None, None, C.c_size_t(0), C.byref(n)) == 0 and n.value == total
        assert L.vxrt_get_voxels_device(ctx._h, lo, hi, None, None, C.c_size_t(0), C.byref(n)) == 0 and n.value == in_box
        assert L.vxrt_get_voxels_device(ctx._h, lo, None, None, None, C.c_size_t(0), C.byref(n)) == H.E_INVALID
        # cap < count: *n is the count, nothing is written
        pos = torch.full((total + 8, 3), 0x5A5A, dtype=torch.int16, device=DEV)
        mrgb = torch.full((total + 8, 4), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        ptr = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
        for cap in (0, 1, total - 1):
            n = C.c_size_t(0)
            assert L.vxrt_get_voxels_device(ctx._h, None, None, ptr(pos), ptr(mrgb), C.c_size_t(cap), C.byref(n)) == H.E_INVALID
            assert n.value == total
            assert bool((pos == 0x5A5A).all()) and bool((mrgb == 0xA5).all()), cap
        # room to spare: exactly the count is written
        assert L.vxrt_get_voxels_device(ctx._h, None, None, ptr(pos), ptr(mrgb), C.c_size_t(total + 8), C.byref(n)) == 0 and n.value == total
        assert np.array_equal(pos[:total].cpu().numpy(), want_p) and np.array_equal(mrgb[:total].cpu().numpy(), want_m)
        assert bool((pos[total:] == 0x5A5A).all()) and bool((mrgb[total:] == 0xA5).all())
        # a destination the kernel's 4-byte stores do not fit (mrgb at an odd byte): the same bytes, through the staging copy
        flat = torch.full((4 * total + 16,), 0xA5, dtype=torch.uint8, device=DEV)
        odd = flat[1: 1 + 4 * total].view(total, 4)
        pos.fill_(0x5A5A)
        torch.cuda.synchronize()
        assert L.vxrt_get_voxels_device(ctx._h, None, None, ptr(pos), ptr(odd), C.c_size_t(total), C.byref(n)) == 0 and n.value == total
        assert np.array_equal(pos[:total].cpu().numpy(), want_p) and np.array_equal(odd.cpu().numpy(), want_m)
        assert int(flat[0]) == 0xA5 and bool((flat[1 + 4 * total:] == 0xA5).all())


# ---- round trip on the device ------------------------------------------------------------------------------------------------------
def test_round_trip_of_a_box_on_the_device(H, scenes):
    load, model, cam = scene(H, scenes, "castle")
    dev, host = twins(H, load, cam)
    with dev, host:
        lo, hi = (2, 0, 1), (13, 10, 12)
        shift = np.array([3, -2, 1], np.int16)
        # on the device: read the box, recolour and shift it with torch, clear the old cells, write the new
        p, m = dev.get_voxels_device(lo, hi)
        assert len(p) > 100
        new_p = p + torch.as_tensor(shift, device=DEV)
        new_m = m.clone()
        new_m[:, 1] = 255 - m[:, 1]
        new_m[:, 3] = m[:, 2]
        dev.clear_voxels_device(p)
        dev.edit_voxels_device(new_p, new_m)
        # the twin: the same on the host
        hp, hm = host.get_voxels(lo, hi)
        assert np.array_equal(hp, p.cpu().numpy()) and np.array_equal(hm, m.cpu().numpy())
        new_hp = hp + shift
        new_hm = hm.copy()
        new_hm[:, 1] = 255 - hm[:, 1]
        new_hm[:, 3] = hm[:, 2]
        host.clear_voxels(hp)
        host.edit_voxels(new_hp, new_hm)
        assert_same_state(dev, host, "round trip")
        M.apply(model, hp, None)
        M.apply(model, new_hp, new_hm)
        assert M.from_list(*dev.get_voxels()) == model
        assert_same_frames(H, dev, host, CFG, 8, "round trip")
