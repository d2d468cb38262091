"""GPU: scenes from dense grids in device memory and boxes of a scene read back as grids (include/vxrt_grid.h).  Every comparison is
bit for bit: a grid's scene has the host builder's records and leaf words (vxrt_build_records of its occupied cells as a list), the
stats, cull box and frames of a context given that list by vxrt_set_voxels, and the records vxrt_set_voxels_device makes of it past the
host builder's limit; an exported box equals the model's scatter of vxrt_get_voxels of that box, on every record layout; refused calls
change nothing; producers and consumers on torch's streams are ordered by the Python wrapper."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first: imported here, at collection, before any test loads libvxrt.so
import torch

import grid_model as G
from conftest import reference_vox, reference_vox_names
from test_gpu_device_build import MRGB0, assert_records, assert_same_scene
from test_gpu_edit import CONFIGS, W, H_, assert_same_frames, make_ctx

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def grids_of(pos, mrgb, origin=None, dims=None):
    """-> [(what, cells, palette)]: the WORD32 grid always, the PALETTE8 grid when the list has at most 255 distinct words"""
    if origin is None:
        origin, dims = G.bounding_box(pos)
    out = [("word32", G.list_to_grid(pos, mrgb, origin, dims), None)]
    pg = G.palette_grid(pos, mrgb, origin, dims)
    if pg is not None:
        out.append(("palette8", pg[0], pg[1]))
    return origin, out


def fixture_list(H, name):
    if name == "startup":
        return H.default_scene_voxels(1)
    if name.startswith("sponge"):
        return H.menger_voxels(int(name[-1]), MRGB0)
    pos, mrgb, _ = H.vox_to_voxels(reference_vox(name))
    return pos, mrgb


def camera_for(scenes, pos):
    origin, dims = G.bounding_box(pos)
    return scenes.close_camera(tuple(max(abs(o), abs(o + d)) for o, d in zip(origin, dims)))


@pytest.mark.parametrize("name", reference_vox_names() + ["startup"] + [f"sponge{k}" for k in range(1, 6)])
def test_fixture_scenes_equal_the_host_build(H, name):
    from gpu_voxel_raytracer_amd import scenes
    pos, mrgb = fixture_list(H, name)
    origin, grids = grids_of(pos, mrgb)
    cfg = (1, 1, 1, 1)
    host = make_ctx(H, cfg)
    with host:
        host.recreate_octree(pos, mrgb)
        host.camera = H.Camera(*camera_for(scenes, pos))
        for what, cells, palette in grids:
            with make_ctx(H, cfg) as dev:
                dev.set_voxel_grid(cells, origin, palette)
                assert_records(H, dev, pos, mrgb, f"{name} {what}")
                assert_same_scene(dev, host, f"{name} {what}")
                if not name.startswith("sponge") or name in ("sponge1", "sponge3"):
                    dev.camera = host.camera
                    assert_same_frames(H, dev, host, cfg, 3, f"{name} {what}")


@pytest.mark.parametrize("cfg", CONFIGS)
def test_frames_of_every_config_after_a_previous_scene(H, cfg):
    from gpu_voxel_raytracer_amd import scenes
    pos, mrgb = H.default_scene_voxels(1)
    origin, grids = grids_of(pos, mrgb)
    dev, host = make_ctx(H, cfg), make_ctx(H, cfg)
    with dev, host:
        for c in (dev, host):                                                 # a previous scene with a temporal history
            c.set_menger(2, 0, (0, 200, 10, 10))
            c.camera = H.Camera(*scenes.reference_start_camera())
            c.render(H.ALL)
        host.recreate_octree(pos, mrgb)
        for what, cells, palette in grids:
            dev.set_voxel_grid(cells, origin, palette)
            assert_same_scene(dev, host, what)
            assert_same_frames(H, dev, host, cfg, 5, f"{cfg} {what}")


def check_grid(H, ctx, cells, origin, palette=None, what=""):
    pos, mrgb = G.grid_to_list(cells, origin, palette)
    ctx.set_voxel_grid(cells, origin, palette)
    assert_records(H, ctx, pos, mrgb, what)
    return pos, mrgb


def random_cells(rng, dims, p, word32=True):
    occ = rng.random(dims) < p
    if word32:
        w = (rng.integers(0, 1 << 31, dims, dtype=np.int64) | (1 << 31)).astype(np.uint32)
        return np.where(occ, w, rng.integers(0, 1 << 31, dims).astype(np.uint32)).view(np.int32)   # empty cells hold junk below bit 31
    return np.where(occ, rng.integers(1, 256, dims), 0).astype(np.uint8)


PLACEMENTS = [
    ((-40, -33, -60), (37, 30, 50)),            # the negative octant
    ((-21, -5, -17), (45, 33, 40)),             # straddling 0
    ((3, -7, 11), (35, 19, 29)),                # odd origin, dims no multiple of 16
    ((5, 5, 5), (1, 1, 1)),                     # one cell
    ((-9, 0, -100), (1, 70, 130)),              # 1 x N x N slabs
    ((0, -100, 3), (70, 1, 90)),
    ((-32768, -32768, -32768), (20, 33, 17)),   # the int16 extremes
    ((32768 - 40, 32768 - 17, 32768 - 64), (40, 17, 64)),
    ((-32768, 100, 32768 - 50), (30, 30, 50)),
    ((-1, -1, -1), (2, 2, 2)),                  # depth 0 and small depths
    ((-4, -3, 0), (8, 6, 4)),
    ((-8, -8, -8), (16, 16, 16)),
]


@pytest.mark.parametrize("origin,dims", PLACEMENTS)
def test_placement_edges(H, origin, dims):
    rng = np.random.default_rng(abs(origin[0]) + dims[2])
    palette = rng.integers(0, 256, (256, 4)).astype(np.uint8)
    with H.Context(W, H_) as ctx:
        for p in (0.3, 1.0):
            check_grid(H, ctx, random_cells(rng, dims, p), origin, None, f"{origin} {dims} word32 {p}")
            check_grid(H, ctx, random_cells(rng, dims, p, False), origin, palette, f"{origin} {dims} palette8 {p}")


def test_every_depth(H):
    rng = np.random.default_rng(9)
    with H.Context(W, H_) as ctx:
        for depth in range(16):
            lim = 1 << depth
            dims = (min(2 * lim, 40),) * 3
            origin = (-lim, -lim, lim - dims[2])
            cells = random_cells(rng, dims, 0.2)
            cells[0, 0, 0] = np.int32(-1)                                         # reaches the root cube's corners
            cells[-1, -1, -1] = np.int32(-1)
            pos, _ = check_grid(H, ctx, cells, origin, None, f"depth {depth}")
            assert ctx.stats().octree_depth == depth


def test_empty_and_full_grids(H):
    from gpu_voxel_raytracer_amd import scenes
    empty_p, empty_m = np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    dev, host = make_ctx(H, (1, 1, 1, 1)), make_ctx(H, (1, 1, 1, 1))
    with dev, host:
        for c in (dev, host):
            c.recreate_octree(*H.default_scene_voxels(1))
            c.camera = H.Camera(*scenes.reference_start_camera())
        host.recreate_octree(empty_p, empty_m)
        for cells in (np.zeros((30, 20, 10), np.int32), np.zeros((0, 5, 5), np.int32), np.zeros((4, 4, 4), np.uint8)):
            palette = np.zeros((256, 4), np.uint8) if cells.dtype == np.uint8 else None
            dev.set_voxel_grid(cells, (-3, 2, 1), palette)
            assert_records(H, dev, empty_p, empty_m, f"empty {cells.shape}")
            assert_same_scene(dev, host, "empty")
        assert_same_frames(H, dev, host, (1, 1, 1, 1), 3, "empty")
        full = np.full((48, 33, 40), 0x80A0B0C0, np.uint32).view(np.int32)
        check_grid(H, dev, full, (-20, -10, -30), None, "full")


def test_past_the_host_node_limit(H):
    """A 2048^3 PALETTE8 grid at about 1 % occupancy (about 86 M voxels): the same records as vxrt_set_voxels_device of its list."""
    n = 2048
    gen = torch.Generator(device=DEV)
    gen.manual_seed(4)
    cells = torch.empty((n, n, n), dtype=torch.uint8, device=DEV)
    for x in range(0, n, 128):
        r = torch.rand((128, n, n), generator=gen, device=DEV)
        cells[x:x + 128] = torch.where(r < 0.01, (r * 25500).to(torch.uint8) + 1, torch.zeros((), dtype=torch.uint8, device=DEV))
        del r
    rng = np.random.default_rng(5)
    palette = rng.integers(0, 256, (256, 4)).astype(np.uint8)
    origin = (-1024, -1024, -1024)
    with H.Context(W, H_) as grid, H.Context(W, H_) as lst:
        grid.set_voxel_grid(cells, origin, palette)
        pal = torch.as_tensor(palette, device=DEV)
        pos, mrgb = [], []
        for x in range(0, n, 128):                                            # the list a user builds today, slab by slab
            slab = cells[x:x + 128]
            idx = torch.nonzero(slab)
            mrgb.append(pal[slab[idx[:, 0], idx[:, 1], idx[:, 2]].long()])
            pos.append((idx + torch.tensor((origin[0] + x, origin[1], origin[2]), device=DEV)).to(torch.int16))
            del idx
        pos, mrgb = torch.cat(pos), torch.cat(mrgb)
        lst.set_voxels_device(pos, mrgb)
        nvox = len(pos)
        del pos, mrgb, cells
        torch.cuda.empty_cache()
        assert nvox > 80_000_000
        a, b = grid.read_scene(), lst.read_scene()
        assert len(a[0]) >= 1 << 26
        assert np.array_equal(a[0], b[0]), "records"
        assert np.array_equal(a[1], b[1]), "leaf words"


def export_equals_model(ctx, origin, dims, what=""):
    origin = tuple(int(v) for v in origin)
    dims = tuple(int(v) for v in dims)
    got = ctx.get_voxel_grid(origin, dims).cpu().numpy()
    hi = tuple(min(o + d, 2 ** 31 - 1) for o, d in zip(origin, dims))
    pos, mrgb = ctx.get_voxels(origin, hi)
    want = G.list_to_grid(pos, mrgb, origin, dims)
    assert np.array_equal(got, want), f"{what}: box {origin} + {dims}"


def random_boxes(rng, depth, count):
    lim = 1 << depth
    for _ in range(count):
        origin = rng.integers(-lim - 20, lim + 5, 3)
        dims = rng.integers(1, min(2 * lim + 30, 90), 3)
        yield origin, dims
    yield (-lim, -lim, -lim), (min(2 * lim, 100),) * 3
    yield (lim + 3, 0, 0), (5, 5, 5)                                           # wholly outside the root cube
    yield (-2 ** 31, -2 ** 31, 2 ** 31 - 4), (3, 2, 3)                         # at the int32 extremes


def test_export_random_boxes_and_after_edits(H):
    rng = np.random.default_rng(12)
    pos, mrgb = H.default_scene_voxels(1)
    with H.Context(W, H_) as ctx:
        ctx.recreate_octree(pos, mrgb)
        depth = ctx.stats().octree_depth
        for o, d in random_boxes(rng, depth, 12):
            export_equals_model(ctx, o, d, "startup")
        lim = 1 << depth
        ep = rng.integers(-lim, lim, (3000, 3)).astype(np.int16)
        em = rng.integers(0, 256, (3000, 4)).astype(np.uint8)
        ctx.edit_voxels(ep, em)
        ctx.clear_voxels(pos[::5])
        for o, d in random_boxes(rng, depth, 12):
            export_equals_model(ctx, o, d, "edited")


@pytest.mark.parametrize("order", [2, 3])
def test_export_treelet_orders(H, order):
    rng = np.random.default_rng(order)
    pos, mrgb = H.default_scene_voxels(1)
    with H.Context(W, H_, tuning=[(H.OPT_NODE_ORDER, order)]) as ctx:
        ctx.recreate_octree(pos, mrgb)
        assert ctx.stats().node_order == order
        for o, d in random_boxes(rng, ctx.stats().octree_depth, 10):
            export_equals_model(ctx, o, d, f"order {order}")


def test_export_device_sponges(H):
    rng = np.random.default_rng(13)
    with H.Context(W, H_) as ctx:
        for level, clip in ((3, 0), (4, 70)):
            ctx.set_menger(level, clip, MRGB0, 5)
            for o, d in random_boxes(rng, ctx.stats().octree_depth, 8):
                export_equals_model(ctx, o, d, f"menger {level}")


def test_round_trip_renders_the_same(H):
    from gpu_voxel_raytracer_amd import scenes
    pos, mrgb = H.default_scene_voxels(1)
    origin, dims = G.bounding_box(pos)
    cfg = (1, 1, 1, 1)
    src, dst = make_ctx(H, cfg), make_ctx(H, cfg)
    with src, dst:
        src.recreate_octree(pos, mrgb)
        src.edit_voxels(pos[::9], np.full((len(pos[::9]), 4), 77, np.uint8))   # overwrites: the same cells, other words
        lo, hi = np.asarray(origin), np.add(origin, dims)
        g = src.get_voxel_grid(lo, hi - lo)
        dst.set_voxel_grid(g, tuple(lo))
        for c in (src, dst):
            c.camera = H.Camera(*scenes.reference_start_camera())
        assert all(np.array_equal(a, b) for a, b in zip(src.get_voxels(), dst.get_voxels()))
        assert_same_frames(H, dst, src, cfg, 4, "round trip")


def test_deterministic(H):
    rng = np.random.default_rng(14)
    cells = torch.as_tensor(random_cells(rng, (150, 170, 130), 0.1), device=DEV)
    with H.Context(W, H_) as ctx:
        ctx.set_voxel_grid(cells, (-70, -9, 3))
        first = ctx.read_scene()
        ctx.set_voxel_grid(cells, (-70, -9, 3))
        again = ctx.read_scene()
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


def test_refused_calls_change_nothing(H):
    from gpu_voxel_raytracer_amd import scenes
    cfg = (4, 1, 1, 1)
    pos, mrgb = H.default_scene_voxels(1)
    ctx, ref = make_ctx(H, cfg), make_ctx(H, cfg)
    with ctx, ref:
        for c in (ctx, ref):
            c.recreate_octree(pos, mrgb)
            c.camera = H.Camera(*scenes.reference_start_camera())
            c.render(H.ALL)
        before = ctx.read_scene()
        L = ctx._L
        hip = C.CDLL("libamdhip64.so")                                         # an allocation of its own: its extent is exact
        raw = C.c_void_p()
        assert hip.hipMalloc(C.byref(raw), C.c_size_t(8 * 8 * 8 * 4)) == 0
        dev_w = torch.full((8, 8, 8), -1, dtype=torch.int32, device=DEV)
        dev_p = torch.ones((8, 8, 8), dtype=torch.uint8, device=DEV)
        host_w = np.full((8, 8, 8), -1, np.int32)
        pal = np.ones((256, 4), np.uint8)
        ptr = lambda t: C.c_void_p(t.data_ptr())                                # noqa: E731
        dims = lambda *d: (C.c_uint32 * 3)(*d)                                  # noqa: E731
        org = lambda *o: (C.c_int32 * 3)(*o)                                    # noqa: E731
        P8, W32 = C.c_int(H.GRID_PALETTE8), C.c_int(H.GRID_WORD32)
        ppal = pal.ctypes.data_as(C.c_void_p)
        calls = [
            (host_w.ctypes.data_as(C.c_void_p), W32, dims(8, 8, 8), org(0, 0, 0), None),       # host memory
            (raw, W32, dims(8, 8, 9), org(0, 0, 0), None),                                     # past the allocation
            (ptr(dev_p), P8, dims(8, 8, 8), org(0, 0, 0), None),                               # PALETTE8 without a palette
            (ptr(dev_w), W32, dims(8, 8, 8), org(0, 0, 0), ppal),                              # WORD32 with one
            (ptr(dev_w), C.c_int(3), dims(8, 8, 8), org(0, 0, 0), None),                       # a bad format
            (ptr(dev_w), C.c_int(0), dims(8, 8, 8), org(0, 0, 0), None),
            (ptr(dev_w), W32, dims(8, 8, 8), org(-32769, 0, 0), None),                         # outside int16
            (ptr(dev_w), W32, dims(8, 8, 8), org(0, 32761, 0), None),
            (None, W32, dims(8, 8, 8), org(0, 0, 0), None),                                    # null cells
        ]
        torch.cuda.synchronize()
        for i, (cells, fmt, d, o, p) in enumerate(calls):
            assert L.vxrt_set_voxel_grid(ctx._h, cells, fmt, d, o, p) == H.E_INVALID, i
            after = ctx.read_scene()
            assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1]), i
        # the edges of the int16 range are accepted
        assert L.vxrt_set_voxel_grid(ref._h, ptr(dev_w), W32, dims(8, 8, 8), org(0, 32760, -32768), None) == 0
        ref.recreate_octree(pos, mrgb)
        assert_same_scene(ctx, ref, "refused")
        assert_same_frames(H, ctx, ref, cfg, 6, "refused")
        # export refusals: host memory, past the allocation
        assert L.vxrt_get_voxel_grid(ctx._h, org(0, 0, 0), dims(8, 8, 8), host_w.ctypes.data_as(C.c_void_p)) == H.E_INVALID
        assert L.vxrt_get_voxel_grid(ctx._h, org(0, 0, 0), dims(8, 8, 9), raw) == H.E_INVALID
        assert hip.hipFree(raw) == 0


def test_producer_on_a_side_stream_is_ordered(H):
    rng = np.random.default_rng(15)
    cells = random_cells(rng, (200, 200, 200), 0.2)
    pos, mrgb = G.grid_to_list(cells, (0, 0, 0))
    src = torch.as_tensor(cells, device=DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with H.Context(W, H_) as ctx:
        with torch.cuda.stream(side):
            t = torch.zeros_like(src)
            torch.cuda._sleep(50_000_000)            # the producer is still busy when the build is asked for
            t.copy_(src)
            ctx.set_voxel_grid(t, (0, 0, 0))
        assert_records(H, ctx, pos, mrgb, "side stream")


def test_export_is_ordered_for_the_next_torch_op(H):
    rng = np.random.default_rng(16)
    cells = random_cells(rng, (256, 256, 256), 0.3)
    want = int(np.count_nonzero(cells.view(np.uint32) >> 31))
    with H.Context(W, H_) as ctx:
        ctx.set_voxel_grid(cells, (-128, -128, -128))
        for _ in range(3):
            torch.cuda._sleep(20_000_000)                                     # torch's stream is busy when the export is asked for
            out = torch.full((256, 256, 256), 5, dtype=torch.int32, device=DEV)
            g = ctx.get_voxel_grid((-128, -128, -128), (256, 256, 256), out=out)
            got = int((g < 0).sum().item())                                   # a torch op right after the call, no explicit sync
            assert got == want
            assert int((g == 5).sum().item()) == 0
