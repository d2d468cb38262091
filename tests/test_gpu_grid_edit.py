"""GPU: a dense grid written into a box of a loaded scene (include/vxrt_grid_edit.h).  The call is defined as vxrt_edit_voxels(clears)
then vxrt_edit_voxels(sets) of the lists tests/grid_edit_model.py derives, so every check compares a context given the grid against a
twin given those two calls: the records and leaf words in use, vxrt_stats with the cull box, the counts, the decoded scene, the box
read back, and the frames with their temporal history — all bit for bit.  Refused calls change nothing; producers on torch's streams
are ordered by the wrapper."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first: imported here, at collection, before any test loads libvxrt.so
import torch

import edit_model as M
import grid_edit_model as GE
import grid_model as G
from conftest import assert_bits_equal
from test_gpu_device_build import MRGB0, assert_same_scene
from test_gpu_edit import BOUNCES, CONFIGS, W, H_, make_ctx, trace_images

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FORMATS = ("word32", "palette8")
MODES = ("replace", "set", "clear")


def small_scene(depth, seed):
    """a random scene that fills part of the root cube of `depth` (and pins that depth)"""
    rng = np.random.default_rng(seed)
    h = 1 << depth
    pos = np.unique(rng.integers(-h, h, (max(4, (2 * h) ** 3 // 3), 3)), axis=0)
    pos = np.concatenate([pos, [[-h, -h, -h]]]).astype(np.int16)
    pos = np.unique(pos, axis=0)
    return pos, rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)


def scene(H, scenes, name):
    """-> (loader(ctx), model dict, camera, depth)"""
    if name == "sponge_device":      # vxrt_set_voxels_device of a level-3 sponge: no host build of it
        pos, mrgb = H.menger_voxels(3, MRGB0)
        load = lambda c: c.set_voxels_device(pos, mrgb)   # noqa: E731
        cam = scenes.close_camera((27, 27, 27))
    elif name == "empty":
        pos, mrgb = np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
        load = lambda c: c.recreate_octree(pos, mrgb)   # noqa: E731
        cam = scenes.close_camera((2, 2, 2))
    elif name.startswith("small"):   # depth < 4: the root cube is one tile that is not 16-aligned
        pos, mrgb = small_scene(int(name[-1]), 5)
        load = lambda c: c.recreate_octree(pos, mrgb)   # noqa: E731
        cam = scenes.close_camera((16, 16, 16))
    elif name == "startup":
        pos, mrgb = H.default_scene_voxels(1)
        load = lambda c: c.recreate_octree(pos, mrgb)   # noqa: E731
        cam = scenes.reference_start_camera()
    else:
        pos, mrgb, size = scenes.load_scene(name)
        load = lambda c: c.recreate_octree(pos, mrgb)   # noqa: E731
        cam = scenes.close_camera(size)
    depth = H.build_octree(pos, mrgb)[1] if len(pos) else 0
    return load, M.from_list(pos, mrgb), cam, depth


def boxes(depth, model):
    """the issue's box kinds for a scene of `depth`: 16-aligned, unaligned, one cell, straddling the root cube's faces, the whole cube"""
    h = 1 << depth
    keys = np.array(sorted(model), np.int64).reshape(-1, 3)
    mid = tuple(int(v) for v in keys[len(keys) // 2]) if len(keys) else (0, 0, 0)
    a = [max(-h, (v // 16) * 16 - 16) for v in mid]
    yield "aligned", tuple(a), (32, 16, 48)
    yield "unaligned", tuple(v - 7 for v in mid), (21, 13, 30)
    yield "one cell", mid, (1, 1, 1)
    yield "straddling", (h - 5, -h - 4, mid[2] - 3), (9, 11, 7)
    if depth <= 6:
        yield "whole cube", (-h, -h, -h), (2 * h, 2 * h, 2 * h)


def make_grid(rng, model, origin, dims, depth, fmt, mode):
    """A grid for the box: mostly the scene's own cells (unchanged), some cleared, recoloured or new; under SET / REPLACE nothing
    occupied outside the root cube.  -> (cells, palette or None)"""
    s = GE.box_words(model, origin, dims)
    r = rng.random(dims)
    new_words = (rng.integers(0, 1 << 31, dims) | (1 << 31)).astype(np.uint32).view(np.int32).astype(np.int64)
    g = np.where(r < 0.15, 0, s)                             # cleared
    g = np.where((r >= 0.15) & (r < 0.25), new_words, g)     # recoloured or new
    if mode == "clear":                                      # carve: occupied where to clear, also over empty cells
        g = np.where(r < 0.5, new_words, 0)
    inside = GE.in_cube(origin, dims, depth)
    if mode != "clear":
        g = np.where(inside, g, 0)
    if fmt == "word32":
        junk = rng.integers(0, 1 << 31, dims)                 # empty cells hold junk below bit 31
        return np.where(g != 0, g, junk).astype(np.int64).astype(np.uint32).view(np.int32), None
    # PALETTE8: the box's most common words in the palette (so most cells stay as they are), the rest mapped to random entries
    words, cnt = np.unique(g[g != 0], return_counts=True)
    top = words[np.argsort(-cnt)][:200]
    palette = rng.integers(0, 256, (256, 4)).astype(np.uint8)
    palette[0] = 0
    palette[1:1 + len(top)] = GE.mrgb_of_words(top)
    order = np.argsort(top)
    at = np.clip(np.searchsorted(top[order], g), 0, max(len(top) - 1, 0))
    idx = rng.integers(1, 256, dims)
    if len(top):
        hit = top[order][at] == g
        idx = np.where(hit, order[at] + 1, idx)
    return np.where(g != 0, idx, 0).astype(np.uint8), palette


def twin_edit(twin, model, cells, origin, mode, depth, palette):
    """the definition on the twin: vxrt_edit_voxels(clears) then vxrt_edit_voxels(sets) -> (counts, the model after it)"""
    cpos, spos, swords, out = GE.edit_lists(model, cells, origin, mode, depth, palette)
    if len(cpos):
        twin.clear_voxels(cpos)
    if len(spos):
        twin.edit_voxels(spos, GE.mrgb_of_words(swords))
    return (len(spos), len(cpos)), out


def to_device(cells):
    return torch.as_tensor(np.ascontiguousarray(cells), device=DEV)


def assert_twins(H, a, b, model, depth, origin, dims, what):
    assert_same_scene(a, b, what)
    svo, leaves = a.read_scene()
    assert M.decode_records(svo, leaves, depth) == model, f"{what}: decoded scene"
    got = a.get_voxel_grid(origin, dims).cpu().numpy()
    assert np.array_equal(got, GE.box_of(model, origin, dims)), f"{what}: box read back"


# ---- twin equality ---------------------------------------------------------------------------------------------------------------
SCENES = ["menger", "castle", "startup", "sponge_device", "small2", "small3", "empty"]


@pytest.mark.parametrize("name", SCENES)
def test_grid_edit_equals_the_two_list_edits(H, scenes, name):
    load, model0, cam, depth = scene(H, scenes, name)
    for k, (label, origin, dims) in enumerate(boxes(depth, model0)):
        rng = np.random.default_rng(100 + k)
        model = dict(model0)
        with make_ctx(H, (1, 1, 1, 1)) as a, make_ctx(H, (1, 1, 1, 1)) as b:
            load(a)
            load(b)
            assert a.stats().octree_depth == depth
            for fmt in FORMATS:
                for mode in MODES:
                    what = f"{name} {label} {fmt} {mode}"
                    cells, palette = make_grid(rng, model, origin, dims, depth, fmt, mode)
                    got = a.edit_voxel_grid(to_device(cells), origin, palette, mode)
                    want, model = twin_edit(b, model, cells, origin, mode, depth, palette)
                    assert got == want, what
                    assert_twins(H, a, b, model, depth, origin, dims, what)


# ---- frames with history ----------------------------------------------------------------------------------------------------------
def render_history(H, ctx, cfg, frame):
    ctx.set_frame_number(frame)
    if cfg[3] > 1:
        ctx.render_frames(H.ALL, cfg[3])
    else:
        ctx.render(H.ALL)
        ctx.render(H.ALL)


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "tracer%d-cull%d-fif%d-fpl%d" % c)
@pytest.mark.parametrize("name", ["castle", "menger"])
def test_frames_with_history_equal_the_twin(H, scenes, name, cfg):
    load, model, cam, depth = scene(H, scenes, name)
    rng = np.random.default_rng(7)
    keys = np.array(sorted(model), np.int64)
    origin = tuple(int(v) - 10 for v in keys[len(keys) // 2])
    dims = (24, 20, 28)
    with make_ctx(H, cfg) as a, make_ctx(H, cfg) as b:
        for c in (a, b):
            load(c)
            c.camera = H.Camera(*cam)
            render_history(H, c, cfg, 1)                      # a temporal history that the edit keeps
        for step, mode in enumerate(("replace", "set", "clear")):
            cells, palette = make_grid(rng, model, origin, dims, depth, "word32", mode)
            got = a.edit_voxel_grid(to_device(cells), origin, palette, mode)
            want, model = twin_edit(b, model, cells, origin, mode, depth, palette)
            assert got == want and sum(got) > 0
            assert_same_scene(a, b, f"{name} {mode}")
            render_history(H, a, cfg, 10 + 5 * step)
            render_history(H, b, cfg, 10 + 5 * step)
            for i in (H.ACCUM_COLOR, H.DENOISED):
                assert_bits_equal(a.read(i), b.read(i), f"{name} {cfg} {mode}: pipeline image {i}")
            assert np.array_equal(a.read(H.DISPLAY_RGBA8_SRGB), b.read(H.DISPLAY_RGBA8_SRGB)), f"{name} {cfg} {mode}: display"
            for i, (x, y) in enumerate(zip(trace_images(H, a, cfg, 40 + step), trace_images(H, b, cfg, 40 + step))):
                assert_bits_equal(x, y, f"{name} {cfg} {mode}: trace image {i}")


# ---- round trip ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["castle", "menger"])
def test_round_trip_changes_nothing(H, scenes, name):
    cfg = (4, 1, 1, 1)
    load, model, cam, depth = scene(H, scenes, name)
    h = 1 << depth
    with make_ctx(H, cfg) as ctx:
        load(ctx)
        ctx.camera = H.Camera(*cam)
        ctx.edit_voxels([[-h, -h, -h]], [[1, 2, 3, 4]])        # an edited scene: blocks of 8 entries past the build's counts
        before = ctx.read_scene()
        stats = ctx.stats()
        images = trace_images(H, ctx, cfg, 3)
        for origin, dims in (((-h, -h, -h), (2 * h,) * 3), ((3, -5, 7), (40, 33, 17)), ((h - 4, h - 4, h - 4), (9, 9, 9))):
            cells = ctx.get_voxel_grid(origin, dims)
            assert ctx.edit_voxel_grid(cells, origin) == (0, 0), (origin, dims)
            after = ctx.read_scene()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
            assert ctx.stats().octree_nodes == stats.octree_nodes
            assert list(ctx.stats().cull_box_min) == list(stats.cull_box_min)
        for i, (x, y) in enumerate(zip(trace_images(H, ctx, cfg, 3), images)):
            assert_bits_equal(x, y, f"{name}: trace image {i} after the round trips")


# ---- a sequence of torch modifications ---------------------------------------------------------------------------------------------
def modify(step, t, gen):
    """one torch modification of an int32 box of leaf words (on the GPU) -> (cells, mode)"""
    n = t.shape
    idx = torch.stack(torch.meshgrid(*[torch.arange(v, device=t.device) for v in n], indexing="ij"), -1).float()
    centre = torch.rand(3, generator=gen, device=t.device) * torch.tensor(n, device=t.device).float()
    radius = float(torch.randint(2, 9, (1,), generator=gen, device=t.device))
    ball = ((idx - centre) ** 2).sum(-1) <= radius * radius
    colour = int(torch.randint(0, 1 << 31, (1,), generator=gen, device=t.device)) | (1 << 31)
    colour = colour - (1 << 32)                                       # as int32
    kind = step % 4
    if kind == 0:                                                      # a brush: paint a ball
        return torch.where(ball, torch.full_like(t, colour), t), "replace"
    if kind == 1:                                                      # carve a ball
        return torch.where(ball, torch.full_like(t, colour), torch.zeros_like(t)), "clear"
    if kind == 2:                                                      # a cellular-automaton-like step: grow into empty neighbours
        occ = (t < 0).float()[None, None]
        near = torch.nn.functional.max_pool3d(occ, 3, 1, 1)[0, 0] > 0
        grow = near & (t >= 0) & (torch.rand(n, generator=gen, device=t.device) < 0.3)
        return torch.where(grow, torch.full_like(t, colour), torch.zeros_like(t)), "set"
    noise = torch.rand(n, generator=gen, device=t.device) < 0.05      # destruction: random cells drop out
    return torch.where(noise, torch.zeros_like(t), t), "replace"


def test_twenty_steps_of_torch_modifications(H, scenes):
    load, model, cam, depth = scene(H, scenes, "castle")
    origin, dims = (-3, 2, 4), (30, 26, 40)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(20)
    with make_ctx(H, (4, 1, 1, 1)) as a, make_ctx(H, (4, 1, 1, 1)) as again, make_ctx(H, (4, 1, 1, 1)) as b:
        for c in (a, again, b):
            load(c)
            c.camera = H.Camera(*cam)
        for step in range(20):
            box = a.get_voxel_grid(origin, dims)
            cells, mode = modify(step, box, gen)
            cells = torch.where(torch.as_tensor(GE.in_cube(origin, dims, depth), device=DEV), cells, torch.zeros_like(cells))
            got = a.edit_voxel_grid(cells, origin, mode=mode)
            assert again.edit_voxel_grid(cells, origin, mode=mode) == got
            want, model = twin_edit(b, model, cells.cpu().numpy(), origin, mode, depth, None)
            assert got == want, step
            assert_same_scene(a, b, f"step {step}")
            assert_same_scene(a, again, f"step {step}: a second context")
            assert np.array_equal(a.get_voxel_grid(origin, dims).cpu().numpy(), GE.box_of(model, origin, dims)), step
        for i, (x, y) in enumerate(zip(trace_images(H, a, (4, 1, 1, 1), 5), trace_images(H, b, (4, 1, 1, 1), 5))):
            assert_bits_equal(x, y, f"after 20 steps: trace image {i}")


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def raw(ctx, cells, fmt, dims, origin, palette, mode, counts=None):
    return ctx._L.vxrt_edit_voxel_grid(ctx._h, C.c_void_p(cells), C.c_int(fmt), (C.c_uint32 * 3)(*dims), (C.c_int32 * 3)(*origin),
                                       None if palette is None else palette.ctypes.data_as(C.c_void_p), C.c_int(mode), counts)


def test_refusals_change_nothing(H, scenes):
    load, model, cam, depth = scene(H, scenes, "castle")
    h = 1 << depth
    cells = to_device(np.full((8, 8, 8), -1, np.int32))               # every cell occupied
    idx = to_device(np.ones((8, 8, 8), np.uint8))
    pal = np.zeros((256, 4), np.uint8)
    host = np.zeros(512, np.int32)
    W32, P8 = H.GRID_WORD32, H.GRID_PALETTE8
    with make_ctx(H, (1, 1, 1, 1)) as none:
        assert raw(none, cells.data_ptr(), W32, (8, 8, 8), (0, 0, 0), None, 1) == H.E_NOSCENE
    with make_ctx(H, (1, 1, 1, 1)) as ctx:
        load(ctx)
        before = ctx.read_scene()
        counts = (C.c_uint64 * 2)(5, 5)
        cases = [
            (H.E_INVALID, (None, W32, (8, 8, 8), (0, 0, 0), None, 1)),                    # null cells, non-empty box
            (H.E_INVALID, (cells.data_ptr(), 7, (8, 8, 8), (0, 0, 0), None, 1)),          # bad format
            (H.E_INVALID, (cells.data_ptr(), W32, (8, 8, 8), (0, 0, 0), None, 4)),        # bad mode
            (H.E_INVALID, (idx.data_ptr(), P8, (8, 8, 8), (0, 0, 0), None, 1)),           # PALETTE8 without a palette
            (H.E_INVALID, (cells.data_ptr(), W32, (8, 8, 8), (0, 0, 0), pal, 1)),         # WORD32 with one
            (H.E_INVALID, (host.ctypes.data, W32, (8, 8, 8), (0, 0, 0), None, 1)),        # host memory
            (H.E_INVALID, (cells.data_ptr(), W32, (8, 8, 1 << 22), (0, 0, 0), None, 1)),  # past the allocation (torch's 2 MiB segment)
            (H.E_SCENE, (cells.data_ptr(), W32, (8, 8, 8), (h - 4, 0, 0), None, 1)),      # occupied outside the cube: REPLACE
            (H.E_SCENE, (cells.data_ptr(), W32, (8, 8, 8), (0, -h - 1, 0), None, 2)),     # ... and SET
            (H.E_SCENE, (idx.data_ptr(), P8, (8, 8, 8), (0, 0, h - 1), pal, 2)),
        ]
        for status, args in cases:
            assert raw(ctx, *args, counts) == status, args
            assert list(counts) == [0, 0]
            after = ctx.read_scene()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), args
        # CLEAR ignores every cell outside the cube; a box wholly outside changes nothing
        outside = GE.in_cube((h - 4, 0, 0), (8, 8, 8), depth)
        want = sum(1 for (x, y, z) in model if h - 4 <= x < h and 0 <= y < 8 and 0 <= z < 8)
        assert raw(ctx, cells.data_ptr(), W32, (8, 8, 8), (h - 4, 0, 0), None, 3, counts) == 0
        assert list(counts) == [0, want] and outside.sum() == 4 * 64
        assert ctx.edit_voxel_grid(cells, (h + 10, 0, 0), mode="clear") == (0, 0)
        assert ctx.edit_voxel_grid(cells[:0], (0, 0, 0)) == (0, 0)
    with make_ctx(H, (1, 1, 1, 1), tuning=[(H.OPT_NODE_ORDER, 2)]) as tre:
        load(tre)
        before = tre.read_scene()
        assert raw(tre, cells.data_ptr(), W32, (8, 8, 8), (0, 0, 0), None, 1) == H.E_INVALID
        after = tre.read_scene()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


# ---- ordering ------------------------------------------------------------------------------------------------------------------
def test_producer_on_a_side_stream_is_ordered(H, scenes):
    load, model, cam, depth = scene(H, scenes, "castle")
    origin, dims = (0, 0, 0), (64, 32, 64)
    rng = np.random.default_rng(3)
    cells, _ = make_grid(rng, model, origin, dims, depth, "word32", "replace")
    src = to_device(cells)
    side = torch.cuda.Stream(DEV)
    with make_ctx(H, (1, 1, 1, 1)) as a, make_ctx(H, (1, 1, 1, 1)) as b:
        load(a)
        load(b)
        with torch.cuda.stream(side):
            t = torch.zeros_like(src)
            torch.cuda._sleep(50_000_000)            # the producer is still busy when the edit is asked for
            t.copy_(src)
            got = a.edit_voxel_grid(t, origin)
        want, model = twin_edit(b, model, cells, origin, "replace", depth, None)
        assert got == want
        assert_twins(H, a, b, model, depth, origin, dims, "side stream")


# ---- multi-GPU ---------------------------------------------------------------------------------------------------------------------
def test_two_ranks_apply_the_same_call(H, scenes):
    load, model, cam, depth = scene(H, scenes, "castle")
    rng = np.random.default_rng(9)
    origin, dims = (-2, 3, 1), (25, 18, 22)
    cells, _ = make_grid(rng, model, origin, dims, depth, "word32", "replace")
    with make_ctx(H, (4, 1, 1, 1)) as single:
        ranks = [H.Context(W, H_, max_bounces=BOUNCES, tracer=4, rank=r, nranks=2, band_rows=16) for r in range(2)]
        try:
            got = []
            for c in [single] + ranks:
                load(c)
                c.camera = H.Camera(*cam)
                got.append(c.edit_voxel_grid(to_device(cells), origin))
                c.set_frame_number(6)
                c.render(H.TRACE)
            assert got[0] == got[1] == got[2] and sum(got[0]) > 0
            for c in ranks:
                assert_same_scene(c, single, "rank")
                assert_bits_equal(c.read(H.SAMPLED_COLOR), single.read(H.SAMPLED_COLOR)[c.local_rows()], "rank rows")
        finally:
            for c in ranks:
                c.close()
