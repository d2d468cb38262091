"""GPU: a triangle mesh voxelised on the device into a device voxel list (include/vxrt_voxelize.h).  Every comparison is bit for bit
against the numpy model of the rule (voxelize_model.py): positions, mrgb bytes, order and count.  Refused calls write nothing; the call
touches no scene; set_mesh / edit_mesh leave what the model's list leaves through the host calls."""
import ctypes as C
import functools

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import voxelize_model as M
from conftest import assert_bits_equal
from test_gpu_device_build import assert_same_scene
from test_gpu_edit import make_ctx, trace_images

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
CFG = (4, 1, 1, 1)
ONE = (3, 0xB0, 0xD0, 0x60)
TABLE = M.table()
GUARD_POS, GUARD_MRGB = 0x5A5A, 0xA5


def sixteenths(verts):
    """the vertices on the snapping grid, so that translating them by whole voxels is exact in binary32"""
    return (np.rint(verts.astype(np.float64) * 16) / 16).astype(np.float32)


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (verts, tris, mrgb [t, 4]) of a named mesh; the model's list of each is computed once (expected)"""
    if name in TABLE:
        v, t = TABLE[name][0]
        return v, t, np.broadcast_to(np.array(ONE, np.uint8), (len(t), 4)).copy()
    if name == "all":               # every mesh of the table in one, a colour per triangle: overlaps between meshes, and the two
        return M.concatenated([m for m, _ in TABLE.values()])     # large triangles among hundreds of small ones
    if name == "icosphere4":
        v, t = M.icosphere(4)
        k = np.arange(len(t))
        return v, t, np.stack([k % 128, k % 256, (k // 7) % 256, (k // 256) % 256], axis=1).astype(np.uint8)
    if name.startswith("moved"):
        v, t = TABLE["icosphere2"][0]
        shift = {"moved_x": (-32000, 0, 0), "moved_yz": (0, 32000, -32000), "moved_0": (0, 0, 0), "moved_far": (300, 0, 0)}[name]
        return sixteenths(v) + np.array(shift, np.float32), t, np.broadcast_to(np.array(ONE, np.uint8), (len(t), 4)).copy()
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, n_tris=None):
    v, t, m = mesh(name)
    pos, mrgb = M.voxelize(v, t[:n_tris], m[:n_tris])
    pos.setflags(write=False)
    mrgb.setflags(write=False)
    return pos, mrgb


@pytest.fixture(scope="module")
def ctx(H):
    with make_ctx(H, CFG) as c:      # no scene is loaded: the voxeliser needs none
        yield c


def on_device(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def assert_list(got, want, what):
    pos, mrgb = got
    assert pos.device == DEV and mrgb.device == DEV and pos.dtype == torch.int16 and mrgb.dtype == torch.uint8, what
    assert tuple(pos.shape) == (len(want[0]), 3) and tuple(mrgb.shape) == (len(want[0]), 4), (what, tuple(pos.shape), len(want[0]))
    assert np.array_equal(pos.cpu().numpy(), want[0]), f"{what}: positions"
    assert np.array_equal(mrgb.cpu().numpy(), want[1]), f"{what}: mrgb"


def raw(ctx, verts, tris, mrgb, pos, out, cap):
    """The C call over device tensors / raw addresses -> (status, *n)."""
    ptr = lambda a: a if a is None or isinstance(a, C.c_void_p) else C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a)   # noqa: E731
    n = C.c_size_t(0xDEAD)
    rc = ctx._L.vxrt_voxelize_mesh_device(ctx._h, ptr(verts), C.c_size_t(len(verts)), ptr(tris), ptr(mrgb), C.c_size_t(len(tris)), ptr(pos), ptr(out),
                                          C.c_size_t(cap), C.byref(n))
    return rc, n.value


def device_mesh(name, n_tris=None):
    v, t, m = mesh(name)
    return on_device(v), on_device(t[:n_tris].view(np.int32)), on_device(m[:n_tris])


def guarded(n):
    pos = torch.full((n, 3), GUARD_POS, dtype=torch.int16, device=DEV)
    out = torch.full((n, 4), GUARD_MRGB, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    return pos, out


def untouched(pos, out):
    return bool((pos == GUARD_POS).all()) and bool((out == GUARD_MRGB).all())


# ---- equal to the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TABLE))
def test_the_table_meshes(ctx, name):
    v, t, m = mesh(name)
    want = expected(name)
    assert len(want[0]) == TABLE[name][1]
    assert_list(ctx.voxelize_mesh(v, t, ONE), want, name)                      # numpy in, a single colour broadcast
    assert_list(ctx.voxelize_mesh(*device_mesh(name), cap=len(want[0]) + 3), want, f"{name}, tensors and a cap")


def test_all_meshes_in_one_with_a_colour_per_triangle(ctx):
    v, t, m = mesh("all")
    want = expected("all")
    # what the case is for, checked on the model's list: the meshes share voxels (fewer than the table's counts add up to), and the
    # colours of more triangles than one 256-thread block holds survive (each of the 337 triangles has a colour of its own)
    assert len(want[0]) < sum(count for _, count in TABLE.values())
    assert len(np.unique(want[1], axis=0)) > 256
    assert_list(ctx.voxelize_mesh(v, t, m), want, "all")
    assert_list(ctx.voxelize_mesh(v, t.astype(np.int64), m), want, "all, int64 indices")


@pytest.mark.parametrize("name", ["moved_x", "moved_yz"])
def test_a_translated_sphere_gives_the_translated_voxels(ctx, name):
    v, t, m = mesh(name)
    got = ctx.voxelize_mesh(v, t, m)
    assert_list(got, expected(name), name)
    shift = (v[0] - mesh("moved_0")[0][0]).astype(np.int64)
    here = set(map(tuple, (expected("moved_0")[0].astype(np.int64) + shift).tolist()))
    assert here == set(map(tuple, got[0].cpu().numpy().astype(np.int64).tolist()))
    assert len(here) == TABLE["icosphere2"][1]


def test_a_sphere_of_5120_triangles(ctx):
    v, t, m = mesh("icosphere4")
    assert len(t) == 5120
    assert_list(ctx.voxelize_mesh(v, t, m), expected("icosphere4"), "icosphere4")


@pytest.mark.parametrize("n_tris", [0, 1, 255, 256, 257])
def test_triangle_counts_around_a_block(ctx, n_tris):
    v, t, m = mesh("icosphere2")
    want = expected("icosphere2", n_tris)
    assert (len(want[0]) == 0) == (n_tris == 0)
    assert_list(ctx.voxelize_mesh(v, t[:n_tris], m[:n_tris]), want, f"{n_tris} triangles")
    rc, n = raw(ctx, *device_mesh("icosphere2", n_tris), None, None, 0)
    assert rc == 0 and n == len(want[0])


@pytest.mark.parametrize("order", [(0, 1), (1, 0)], ids=["a then b", "b then a"])
def test_duplicate_triangles_take_the_later_colour(ctx, order):
    v, t, _ = mesh("triangle")
    colours = np.array([[9, 1, 2, 3], [0x85, 4, 5, 6]], np.uint8)[list(order)]
    got = ctx.voxelize_mesh(v, np.concatenate([t, t]), colours)
    want = expected("triangle")
    assert np.array_equal(got[0].cpu().numpy(), want[0])
    last = colours[1].copy()
    last[0] &= 0x7f
    assert (got[1].cpu().numpy() == last).all()
    assert_list(got, M.voxelize(v, np.concatenate([t, t]), colours), "duplicates")


# ---- counting, room, alignment -----------------------------------------------------------------------------------------------------
def test_count_only_and_too_little_room(ctx, H):
    dv, dt, dm = device_mesh("all")
    want = expected("all")
    total = len(want[0])
    assert raw(ctx, dv, dt, dm, None, None, 0) == (0, total)
    assert raw(ctx, dv, dt, None, None, None, 0) == (0, total)                 # counting needs no colours
    pos, out = guarded(total + 8)
    for cap in (0, 1, total - 1):                                              # *n is set and nothing is written
        assert raw(ctx, dv, dt, dm, pos, out, cap) == (H.E_INVALID, total)
        assert untouched(pos, out), cap
    with pytest.raises(H.VxrtError) as e:
        ctx.voxelize_mesh(dv, dt, dm, cap=total - 1)
    assert e.value.status == H.E_INVALID and str(total) in str(e.value)
    assert raw(ctx, dv, dt, dm, pos, out, total + 8) == (0, total)             # room to spare: exactly the count is written
    assert_list((pos[:total], out[:total]), want, "room to spare")
    assert untouched(pos[total:], out[total:])
    assert raw(ctx, dv, dt, dm, pos, None, total)[0] == H.E_INVALID            # one array without the other
    assert raw(ctx, dv, dt, None, pos, out, total)[0] == H.E_INVALID           # output without colours
    assert raw(ctx, dv, dt, dm, None, None, 0)[0] == 0


@pytest.mark.parametrize("pos_off, mrgb_off", [(0, 0), (2, 4), (1, 0), (0, 1), (3, 2), (2, 3)])
def test_output_arrays_at_odd_alignments(ctx, pos_off, mrgb_off):
    dv, dt, dm = device_mesh("icosphere2")
    want = expected("icosphere2")
    total = len(want[0])
    flat_p = torch.full((6 * total + 32,), GUARD_MRGB, dtype=torch.uint8, device=DEV)
    flat_m = torch.full((4 * total + 32,), GUARD_MRGB, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    assert flat_p.data_ptr() % 16 == 0 and flat_m.data_ptr() % 16 == 0
    assert raw(ctx, dv, dt, dm, flat_p.data_ptr() + pos_off, flat_m.data_ptr() + mrgb_off, total) == (0, total)
    got_p = flat_p[pos_off: pos_off + 6 * total].cpu().numpy().view(np.int16).reshape(-1, 3)
    got_m = flat_m[mrgb_off: mrgb_off + 4 * total].cpu().numpy().reshape(-1, 4)
    assert np.array_equal(got_p, want[0]) and np.array_equal(got_m, want[1])
    for flat, off, size in ((flat_p, pos_off, 6 * total), (flat_m, mrgb_off, 4 * total)):
        assert bool((flat[:off] == GUARD_MRGB).all()) and bool((flat[off + size:] == GUARD_MRGB).all())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx, H):
    v, t, m = mesh("icosphere2")
    want = expected("icosphere2")
    pos, out = guarded(len(want[0]) + 4)
    dt, dm = on_device(t.view(np.int32)), on_device(m)

    def refused(verts, tris, status, *words):
        for p, o, cap in ((pos, out, len(pos)), (None, None, 0)):
            rc, n = raw(ctx, on_device(verts), on_device(np.ascontiguousarray(tris).view(np.int32)), dm, p, o, cap)
            assert rc == status and n == 0xDEAD, (rc, n)
            text = (ctx._L.vxrt_last_error() or b"").decode()
            assert all(w in text for w in words), text
        assert untouched(pos, out)

    # every refusal is decided before a kernel reads through a bad index
    for bad in (len(v), len(v) + 1, 0x7fffffff, 0xffffffff):
        tt = t.copy()
        tt[len(t) // 2, 1] = bad
        refused(v, tt, H.E_INVALID, "index")
    refused(v[:0], t, H.E_INVALID, "index")                                    # no vertices at all
    used = int(t[100, 2])
    for bad in (np.nan, np.inf, -np.inf):
        vv = v.copy()
        vv[used, 1] = bad
        refused(vv, t, H.E_INVALID, "finite")
    for bad in (32768.0, -32768.0625, 1e30, 3e38):
        vv = v.copy()
        vv[used, 2] = bad
        refused(vv, t, H.E_SCENE, "-524288", "524288")
    vv = v.copy()
    vv[used] = (np.nan, 40000.0, 0.0)
    refused(vv, t, H.E_INVALID)                                                # not finite and outside: invalid
    # an unused vertex is never read: NaN, infinite or far outside
    spare = np.concatenate([v, [[np.nan, np.inf, 1e30]]]).astype(np.float32)
    assert_list(ctx.voxelize_mesh(spare, t, m), want, "an unused vertex")
    # the last sixteenth inside on both sides
    edge = M.single((-32768, 32767.9375, 0), (-32768, 32767.9375, 0), (-32768, 32767.9375, 0))
    assert ctx.voxelize_mesh(*edge, ONE)[0].cpu().numpy().tolist() == [[-32768, 32767, 0]]
    # host memory: pageable and pinned, for each array
    dv = on_device(v)
    pin_v, pin_t, pin_m = torch.as_tensor(v).pin_memory(), torch.as_tensor(t.view(np.int32)).pin_memory(), torch.as_tensor(m).pin_memory()
    pin_p, pin_o = torch.zeros((len(pos), 3), dtype=torch.int16).pin_memory(), torch.zeros((len(pos), 4), dtype=torch.uint8).pin_memory()
    for args in ((pin_v, dt, dm, pos, out), (dv, pin_t, dm, pos, out), (dv, dt, pin_m, pos, out), (dv, dt, dm, pin_p, out), (dv, dt, dm, pos, pin_o)):
        assert raw(ctx, *args, len(pos)) == (H.E_INVALID, 0xDEAD)
    host_v = np.ascontiguousarray(v)
    rc, n = raw(ctx, torch.as_tensor(host_v), dt, dm, pos, out, len(pos))
    assert rc == H.E_INVALID
    # arrays that end past their allocation
    hip = C.CDLL("libamdhip64.so")
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), C.c_size_t(64)) == 0
    assert raw(ctx, dv, dt, dm, small, out, len(pos))[0] == H.E_INVALID
    assert raw(ctx, dv, dt, dm, pos, small, len(pos))[0] == H.E_INVALID
    assert hip.hipFree(small) == 0
    assert untouched(pos, out)
    assert (pin_p == 0).all() and (pin_o == 0).all()
    # ... and the valid mesh is accepted afterwards
    assert raw(ctx, dv, dt, dm, pos, out, len(pos)) == (0, len(want[0]))
    assert_list((pos[:len(want[0])], out[:len(want[0])]), want, "after the refusals")


# ---- ordering, determinism, the scene ------------------------------------------------------------------------------------------------
def test_a_mesh_written_on_a_side_stream_is_read_whole(ctx):
    v, t, m = mesh("icosphere4")
    src_v, src_t, src_m = on_device(v), on_device(t.view(np.int32)), on_device(m)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        tv, tt, tm = torch.zeros_like(src_v), torch.zeros_like(src_t), torch.zeros_like(src_m)
        torch.cuda._sleep(50_000_000)                   # the producer is still busy when the voxeliser is asked
        tv.copy_(src_v)
        tt.copy_(src_t)
        tm.copy_(src_m)
        got = ctx.voxelize_mesh(tv, tt, tm)
    assert_list(got, expected("icosphere4"), "side stream")


def test_two_calls_write_the_same_bytes(ctx, H):
    dv, dt, dm = device_mesh("all")
    a = ctx.voxelize_mesh(dv, dt, dm)
    b = ctx.voxelize_mesh(dv, dt, dm, cap=len(a[0]) + 100)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with make_ctx(H, CFG) as other:
        c = other.voxelize_mesh(dv, dt, dm)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def test_a_loaded_scene_is_not_touched(H, scenes):
    pos, mrgb, size = scenes.load_scene("menger")
    with make_ctx(H, CFG) as c:
        c.recreate_octree(pos, mrgb)
        c.camera = H.Camera(*scenes.close_camera(size))
        images = trace_images(H, c, CFG, 3)
        svo, leaves = c.read_scene()
        t0 = c.stats()
        stats = (t0.octree_depth, t0.octree_nodes, t0.scene_bytes, t0.cull_box_valid, list(t0.cull_box_min), list(t0.cull_box_max))
        assert_list(c.voxelize_mesh(*mesh("all")), expected("all"), "with a scene loaded")
        svo2, leaves2 = c.read_scene()
        t1 = c.stats()
        assert np.array_equal(svo, svo2) and np.array_equal(leaves, leaves2)
        assert stats == (t1.octree_depth, t1.octree_nodes, t1.scene_bytes, t1.cull_box_valid, list(t1.cull_box_min), list(t1.cull_box_max))
        for i, (a, b) in enumerate(zip(trace_images(H, c, CFG, 3), images)):
            assert_bits_equal(a, b, f"a voxelise changes no image: {i}")
        c.render(H.TRACE)                               # a frame enqueued, not waited for, then a voxelise behind it
        assert_list(c.voxelize_mesh(*mesh("icosphere2")), expected("icosphere2"), "behind a frame")


# ---- into the scene ----------------------------------------------------------------------------------------------------------------
def test_set_mesh_equals_the_models_list_through_set_voxels(H, scenes):
    v, t, m = mesh("all")
    want = expected("all")
    with make_ctx(H, CFG) as dev, make_ctx(H, CFG) as host:
        dev.set_mesh(v, t, m)
        host.recreate_octree(*want)
        for c in (dev, host):
            c.camera = H.Camera(*scenes.close_camera((20, 20, 20)))
        assert_same_scene(dev, host, "set_mesh")
        for i, (a, b) in enumerate(zip(trace_images(H, dev, CFG, 5), trace_images(H, host, CFG, 5))):
            assert_bits_equal(a, b, f"set_mesh: trace image {i}")
        for a, b in zip(dev.get_voxels(), want):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name, grow", [("icosphere2", False), ("moved_far", True)])
def test_edit_mesh_equals_the_models_list_through_edit_voxels(H, scenes, name, grow):
    pos, mrgb, size = scenes.load_scene("menger")
    v, t, m = mesh(name)
    want = expected(name)
    with make_ctx(H, CFG) as dev, make_ctx(H, CFG) as host:
        for c in (dev, host):
            c.recreate_octree(pos, mrgb)
            c.camera = H.Camera(*scenes.close_camera(size))
        depth = dev.scene_depth
        if grow:
            with pytest.raises(H.VxrtError) as e:
                dev.edit_mesh(v, t, m)                  # outside the root cube without grow
            assert e.value.status == H.E_SCENE
            assert_same_scene(dev, host, "edit_mesh refused")
        dev.edit_mesh(v, t, m, grow=grow)
        host.edit_voxels(*want, grow=grow)
        assert (dev.scene_depth > depth) == grow and dev.scene_depth == host.scene_depth
        assert_same_scene(dev, host, f"edit_mesh {name}")
        for i, (a, b) in enumerate(zip(trace_images(H, dev, CFG, 6), trace_images(H, host, CFG, 6))):
            assert_bits_equal(a, b, f"edit_mesh {name}: trace image {i}")
        for a, b in zip(dev.get_voxels(), host.get_voxels()):
            assert np.array_equal(a, b)
