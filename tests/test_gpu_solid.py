"""GPU: a closed triangle mesh voxelised on the device as a solid (include/vxrt_solid.h).  Every comparison is bit for bit against the
numpy model of the rule (solid_model.py): positions, mrgb bytes, order and count, in both modes.  Refused calls write nothing; the
call touches no scene; set_solid / edit_solid / carve_solid leave what the model's lists leave through the host calls."""
import ctypes as C
import functools

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import solid_model as S
import voxelize_model as M
from conftest import assert_bits_equal
from test_gpu_device_build import assert_same_scene
from test_gpu_edit import make_ctx, trace_images
from test_gpu_voxelize import CFG, DEV, GUARD_MRGB, ONE, assert_list, guarded, on_device, untouched

pytestmark = pytest.mark.gpu

FILL = (0x85, 0x11, 0x22, 0x33)      # the material's top bit is dropped
TABLE = S.table()
MODES = [False, True]                # interior_only
MODE_IDS = ["union", "interior"]


def upright(x, y, z=0.0):
    """a vertical triangle (n_z == 0): it has a surface and crosses no column"""
    return M.single((x, y, z), (x + 2.0, y, z), (x + 1.0, y, z + 3.0))


def tetrahedra(count):
    v, t = S.tetrahedron()
    return [(v + np.array([8.0 * (i % 8), 8.0 * (i // 8 % 8), 8.0 * (i // 64)], np.float32), t) for i in range(count)]


@functools.lru_cache(maxsize=None)
def mesh(name):
    """-> (verts, tris, mrgb [t, 4]) of a named mesh"""
    if name in TABLE:
        v, t = TABLE[name][0]
    elif name == "all":                   # every mesh of the table in one, a colour per triangle: the shells overlap, so parity
        return M.concatenated([m for m, _, _ in TABLE.values()])     # decides, and surface cells of one lie inside another
    elif name == "tall":                  # spans longer than a block that cross block boundaries: 9 columns of 600 cells
        v, t = S.box((0, 0, 0), (3, 3, 600))
    elif name == "slivers_then_cube":     # 300 consecutive triangles without a column, then 12 with 64 each
        v, t = S.join(S.slivers(300), M.cube())
    elif name == "zero_pairs":            # a tilted triangle twice: 400 and more pairs of equal crossings; then a cube further along x
        tri = M.single((0.2, 0.1, 0.3), (30.4, 0.3, 5.2), (0.6, 30.7, 9.1))
        v, t = S.join(tri, tri, S.box(40, 46))
    elif name == "top":                   # the top face at the last sixteenth: its crossing is k = 32768
        v, t = S.box((32764, 32765, 32760), (32767.9375, 32767.9375, 32767.9375))
    elif name == "bottom":
        v, t = S.box((-32768, -32768, -32768), (-32765, -32766, -32764))
    elif name.startswith("count"):        # closed meshes of exactly n triangles: tetrahedra, and vertical triangles to make it up
        n = int(name[5:])
        if n == 0:
            return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.uint32), np.zeros((0, 4), np.uint8)
        v, t = S.join(*(tetrahedra(n // 4) + [upright(70.0 + 4 * i, 1.0) for i in range(n % 4)]))
        assert len(t) == n
    else:
        raise KeyError(name)
    k = np.arange(len(t))
    return v, t, np.stack([k % 128, (k * 7 + 1) % 256, (k * 13 + 2) % 256, (k // 256 + 3) % 256], axis=1).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def expected(name, interior_only):
    v, t, m = mesh(name)
    pos, mrgb = S.solid(v, t, m, FILL, interior_only=interior_only)
    pos.setflags(write=False)
    mrgb.setflags(write=False)
    return pos, mrgb


@pytest.fixture(scope="module")
def ctx(H):
    with make_ctx(H, CFG) as c:      # no scene is loaded: the voxeliser needs none
        yield c


def device_mesh(name):
    v, t, m = mesh(name)
    return on_device(v), on_device(t.view(np.int32)), on_device(m)


def raw(ctx, verts, tris, mrgb, fill, mode, pos, out, cap):
    """The C call over device tensors / raw addresses -> (status, *n)."""
    ptr = lambda a: a if a is None or isinstance(a, C.c_void_p) else C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a)   # noqa: E731
    n = C.c_size_t(0xDEAD)
    fill4 = None if fill is None else (C.c_uint8 * 4)(*fill)
    rc = ctx._L.vxrt_voxelize_solid_device(ctx._h, ptr(verts), C.c_size_t(len(verts)), ptr(tris), ptr(mrgb), C.c_size_t(len(tris)), fill4,
                                           C.c_uint32(mode), ptr(pos), ptr(out), C.c_size_t(cap), C.byref(n))
    return rc, n.value


def last_error(ctx):
    return (ctx._L.vxrt_last_error() or b"").decode()


# ---- equal to the model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interior_only", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", list(TABLE))
def test_the_table_meshes(ctx, name, interior_only):
    v, t, m = mesh(name)
    want = expected(name, interior_only)
    assert len(want[0]) == TABLE[name][2 if interior_only else 1]
    assert_list(ctx.voxelize_solid(v, t, m, FILL, interior_only=interior_only), want, name)
    assert_list(ctx.voxelize_solid(*device_mesh(name), FILL, interior_only=interior_only, cap=len(want[0]) + 3), want, f"{name}, tensors and a cap")
    if interior_only:
        assert_list(ctx.voxelize_solid(v, t, None, FILL, interior_only=True), want, f"{name}, no colours")


def test_the_union_keeps_the_surface_and_its_bytes(ctx):
    v, t, m = mesh("icosphere2")
    pos, out = ctx.voxelize_solid(v, t, m, FILL)
    spos, sout = ctx.voxelize_mesh(v, t, m)
    have = {tuple(p): tuple(b) for p, b in zip(pos.cpu().numpy().tolist(), out.cpu().numpy().tolist())}
    for p, b in zip(spos.cpu().numpy().tolist(), sout.cpu().numpy().tolist()):
        assert have[tuple(p)] == tuple(b)
    rest = [b for p, b in have.items() if p not in set(map(tuple, spos.cpu().numpy().tolist()))]
    assert len(rest) == len(pos) - len(spos) > 0 and set(rest) == {(5, 0x11, 0x22, 0x33)}


@pytest.mark.parametrize("interior_only", MODES, ids=MODE_IDS)
def test_all_meshes_in_one_with_a_colour_per_triangle(ctx, interior_only):
    v, t, m = mesh("all")
    want = expected("all", interior_only)
    if not interior_only:        # the surface beats the fill, the highest index wins, and more colours survive than a block has threads
        surface = M.voxelize(v, t, m)
        assert len(np.unique(want[1], axis=0)) > 256 and len(want[0]) > len(surface[0])
        inner = set(map(tuple, expected("all", True)[0].tolist()))
        assert sum(tuple(p) in inner for p in surface[0].tolist()) > 100
    assert_list(ctx.voxelize_solid(v, t, m, FILL, interior_only=interior_only), want, "all")


@pytest.mark.parametrize("interior_only", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", ["tall", "slivers_then_cube", "zero_pairs", "top", "bottom"])
def test_the_meshes_that_stress_the_offsets(ctx, name, interior_only):
    v, t, m = mesh(name)
    want = expected(name, interior_only)
    inner = expected(name, True)[0]
    assert len(inner) == {"tall": 5400, "slivers_then_cube": 512, "zero_pairs": 216, "top": 4 * 3 * 8, "bottom": 3 * 2 * 4}[name]
    if name == "top":
        assert inner[:, 2].max() == 32767
    if name == "bottom":
        assert inner.min() == -32768
    assert_list(ctx.voxelize_solid(v, t, m, FILL, interior_only=interior_only), want, name)


@pytest.mark.parametrize("n_tris", [0, 1, 255, 256, 257])
def test_triangle_counts_around_a_block(ctx, H, n_tris):
    v, t, m = mesh(f"count{n_tris}")
    for interior_only in MODES:
        want = expected(f"count{n_tris}", interior_only)
        assert_list(ctx.voxelize_solid(v, t, m, FILL, interior_only=interior_only), want, f"{n_tris} triangles")
        rc, n = raw(ctx, *device_mesh(f"count{n_tris}"), FILL, int(interior_only), None, None, 0)
        assert rc == 0 and n == len(want[0])
    assert len(expected(f"count{n_tris}", True)[0]) == 38 * (n_tris // 4)
    # open meshes of as many triangles: the first n of the sphere (its first alone lies between the column centres and crosses
    # nothing, so the table's lone triangle of the surface tests stands in for it)
    sv, st, sm = mesh("icosphere2")
    if n_tris == 1:
        sv, st = M.table()["triangle"][0]
    if n_tris:
        with pytest.raises(S.Refused) as model:
            S.interior(sv, st[:n_tris])
        for interior_only in MODES:
            with pytest.raises(H.VxrtError) as e:
                ctx.voxelize_solid(sv, st[:n_tris], sm[:n_tris], FILL, interior_only=interior_only)
            assert e.value.status == H.E_SCENE and f"column ({model.value.column[0]}, {model.value.column[1]})" in str(e.value)
    else:
        assert len(ctx.voxelize_solid(sv, st[:0], sm[:0], FILL)[0]) == 0


# ---- counting, room, alignment -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interior_only", MODES, ids=MODE_IDS)
def test_count_only_and_too_little_room(ctx, H, interior_only):
    dv, dt, dm = device_mesh("all")
    mode = int(interior_only)
    want = expected("all", interior_only)
    total = len(want[0])
    assert raw(ctx, dv, dt, dm, FILL, mode, None, None, 0) == (0, total)
    assert raw(ctx, dv, dt, None, None, mode, None, None, 0) == (0, total)     # counting needs neither colours nor a fill
    pos, out = guarded(total + 8)
    for cap in (0, 1, total - 1):                                              # *n is set and nothing is written
        assert raw(ctx, dv, dt, dm, FILL, mode, pos, out, cap) == (H.E_INVALID, total)
        assert untouched(pos, out), cap
    with pytest.raises(H.VxrtError) as e:
        ctx.voxelize_solid(dv, dt, dm, FILL, interior_only=interior_only, cap=total - 1)
    assert e.value.status == H.E_INVALID and str(total) in str(e.value)
    assert raw(ctx, dv, dt, dm, FILL, mode, pos, out, total + 8) == (0, total)  # room to spare: exactly the count is written
    assert_list((pos[:total], out[:total]), want, "room to spare")
    assert untouched(pos[total:], out[total:])
    assert raw(ctx, dv, dt, dm, FILL, mode, pos, None, total)[0] == H.E_INVALID            # one array without the other
    assert raw(ctx, dv, dt, dm, FILL, mode, None, out, total)[0] == H.E_INVALID


@pytest.mark.parametrize("pos_off, mrgb_off", [(0, 0), (2, 4), (1, 0), (0, 1), (3, 2), (2, 3)])
def test_output_arrays_at_odd_alignments(ctx, pos_off, mrgb_off):
    dv, dt, dm = device_mesh("torus")
    for interior_only in MODES:
        want = expected("torus", interior_only)
        total = len(want[0])
        flat_p = torch.full((6 * total + 32,), GUARD_MRGB, dtype=torch.uint8, device=DEV)
        flat_m = torch.full((4 * total + 32,), GUARD_MRGB, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        assert flat_p.data_ptr() % 16 == 0 and flat_m.data_ptr() % 16 == 0
        assert raw(ctx, dv, dt, dm, FILL, int(interior_only), flat_p.data_ptr() + pos_off, flat_m.data_ptr() + mrgb_off, total) == (0, total)
        got_p = flat_p[pos_off: pos_off + 6 * total].cpu().numpy().view(np.int16).reshape(-1, 3)
        got_m = flat_m[mrgb_off: mrgb_off + 4 * total].cpu().numpy().reshape(-1, 4)
        assert np.array_equal(got_p, want[0]) and np.array_equal(got_m, want[1])
        for flat, off, size in ((flat_p, pos_off, 6 * total), (flat_m, mrgb_off, 4 * total)):
            assert bool((flat[:off] == GUARD_MRGB).all()) and bool((flat[off + size:] == GUARD_MRGB).all())


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_the_mode_the_fill_and_the_colours(ctx, H):
    dv, dt, dm = device_mesh("cube")
    total = {0: len(expected("cube", False)[0]), 1: len(expected("cube", True)[0])}
    pos, out = guarded(total[0] + 4)
    for mode in (2, 3, 0x80000000, 0xffffffff):
        for p, o, cap in ((pos, out, len(pos)), (None, None, 0)):
            assert raw(ctx, dv, dt, dm, FILL, mode, p, o, cap) == (H.E_INVALID, 0xDEAD)
            assert "mode" in last_error(ctx)
        assert raw(ctx, dv[:0], dt[:0], dm[:0], FILL, mode, None, None, 0) == (H.E_INVALID, 0xDEAD)      # even with no triangles
    for mode in (0, 1):
        assert raw(ctx, dv, dt, dm, None, mode, pos, out, len(pos)) == (H.E_INVALID, 0xDEAD)      # a NULL fill with output arrays
        assert "fill" in last_error(ctx)
        assert raw(ctx, dv, dt, dm, None, mode, None, None, 0) == (0, total[mode])                # counting needs none
    assert raw(ctx, dv, dt, None, FILL, 0, pos, out, len(pos)) == (H.E_INVALID, 0xDEAD)           # UNION needs the colours
    assert "tri_mrgb" in last_error(ctx)
    assert untouched(pos, out)
    assert raw(ctx, dv, dt, None, FILL, 1, pos, out, len(pos)) == (0, total[1])                   # INTERIOR does not
    assert_list((pos[:total[1]], out[:total[1]]), expected("cube", True), "INTERIOR without colours")
    # no triangles: 0 without touching a pointer
    assert raw(ctx, dv[:0], dt[:0], None, None, 0, None, None, 0) == (0, 0)
    bad = C.c_void_p(8)
    n = C.c_size_t(0xDEAD)
    assert ctx._L.vxrt_voxelize_solid_device(ctx._h, bad, C.c_size_t(5), bad, bad, C.c_size_t(0), (C.c_uint8 * 4)(*FILL), C.c_uint32(0), bad, bad,
                                             C.c_size_t(9), C.byref(n)) == 0 and n.value == 0


@pytest.mark.parametrize("interior_only", MODES, ids=MODE_IDS)
def test_refusals_write_nothing(ctx, H, interior_only):
    mode = int(interior_only)
    v, t, m = mesh("icosphere2")
    want = expected("icosphere2", interior_only)
    pos, out = guarded(len(want[0]) + 4)
    dt, dm = on_device(t.view(np.int32)), on_device(m)

    def refused(verts, tris, status, *words):
        for p, o, cap in ((pos, out, len(pos)), (None, None, 0)):
            rc, n = raw(ctx, on_device(verts), on_device(np.ascontiguousarray(tris).view(np.int32)), dm[:len(tris)], FILL, mode, p, o, cap)
            assert rc == status and n == 0xDEAD, (rc, n)
            text = last_error(ctx)
            assert all(w in text for w in words), text
        assert untouched(pos, out)

    # every refusal of the surface's call, decided before a kernel reads through a bad index
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
    # the open mesh, with its first odd column and that column's count as the model has them
    hole = np.delete(t, 7, axis=0)
    with pytest.raises(S.Refused) as model:
        S.interior(v, hole)
    refused(v, hole, H.E_SCENE, "not closed", f"column ({model.value.column[0]}, {model.value.column[1]})", f"crossed {model.value.count} times")
    with pytest.raises(S.Refused) as model:
        S.interior(*S.open_cube())
    assert model.value.column == (0, 1)
    refused(*S.open_cube(), H.E_SCENE, "not closed", "column (0, 1)", "crossed 1 times")
    # an unused vertex is never read: NaN, infinite or far outside
    spare = np.concatenate([v, [[np.nan, np.inf, 1e30]]]).astype(np.float32)
    assert_list(ctx.voxelize_solid(spare, t, m, FILL, interior_only=interior_only), want, "an unused vertex")
    # host memory: pageable and pinned, for each array
    dv = on_device(v)
    pin_v, pin_t, pin_m = torch.as_tensor(v).pin_memory(), torch.as_tensor(t.view(np.int32)).pin_memory(), torch.as_tensor(m).pin_memory()
    pin_p, pin_o = torch.zeros((len(pos), 3), dtype=torch.int16).pin_memory(), torch.zeros((len(pos), 4), dtype=torch.uint8).pin_memory()
    for args in ((pin_v, dt, dm, pos, out), (dv, pin_t, dm, pos, out), (dv, dt, pin_m, pos, out), (dv, dt, dm, pin_p, out), (dv, dt, dm, pos, pin_o)):
        assert raw(ctx, *args[:3], FILL, mode, *args[3:], len(pos)) == (H.E_INVALID, 0xDEAD)
    assert raw(ctx, torch.as_tensor(np.ascontiguousarray(v)), dt, dm, FILL, mode, pos, out, len(pos))[0] == H.E_INVALID
    # arrays that end past their allocation
    hip = C.CDLL("libamdhip64.so")
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), C.c_size_t(64)) == 0
    assert raw(ctx, dv, dt, dm, FILL, mode, small, out, len(pos))[0] == H.E_INVALID
    assert raw(ctx, dv, dt, dm, FILL, mode, pos, small, len(pos))[0] == H.E_INVALID
    assert hip.hipFree(small) == 0
    assert untouched(pos, out)
    assert (pin_p == 0).all() and (pin_o == 0).all()
    # ... and the valid mesh is accepted afterwards
    assert raw(ctx, dv, dt, dm, FILL, mode, pos, out, len(pos)) == (0, len(want[0]))
    assert_list((pos[:len(want[0])], out[:len(want[0])]), want, "after the refusals")


# ---- ordering, determinism, the scene ------------------------------------------------------------------------------------------------
def test_a_mesh_written_on_a_side_stream_is_read_whole(ctx):
    v, t, m = mesh("all")
    src_v, src_t, src_m = on_device(v), on_device(t.view(np.int32)), on_device(m)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        tv, tt, tm = torch.zeros_like(src_v), torch.zeros_like(src_t), torch.zeros_like(src_m)
        torch.cuda._sleep(50_000_000)                   # the producer is still busy when the voxeliser is asked
        tv.copy_(src_v)
        tt.copy_(src_t)
        tm.copy_(src_m)
        got = ctx.voxelize_solid(tv, tt, tm, FILL)
    assert_list(got, expected("all", False), "side stream")


def test_two_calls_write_the_same_bytes(ctx, H):
    dv, dt, dm = device_mesh("all")
    for interior_only in MODES:
        a = ctx.voxelize_solid(dv, dt, dm, FILL, interior_only=interior_only)
        b = ctx.voxelize_solid(dv, dt, dm, FILL, interior_only=interior_only, cap=len(a[0]) + 100)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        with make_ctx(H, CFG) as other:
            c = other.voxelize_solid(dv, dt, dm, FILL, interior_only=interior_only)
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
        for interior_only in MODES:
            assert_list(c.voxelize_solid(*mesh("all"), FILL, interior_only=interior_only), expected("all", interior_only), "with a scene loaded")
        svo2, leaves2 = c.read_scene()
        t1 = c.stats()
        assert np.array_equal(svo, svo2) and np.array_equal(leaves, leaves2)
        assert stats == (t1.octree_depth, t1.octree_nodes, t1.scene_bytes, t1.cull_box_valid, list(t1.cull_box_min), list(t1.cull_box_max))
        for i, (a, b) in enumerate(zip(trace_images(H, c, CFG, 3), images)):
            assert_bits_equal(a, b, f"a solid voxelise changes no image: {i}")
        c.render(H.TRACE)                               # a frame enqueued, not waited for, then a voxelise behind it
        assert_list(c.voxelize_solid(*mesh("torus"), FILL), expected("torus", False), "behind a frame")


# ---- into the scene ----------------------------------------------------------------------------------------------------------------
def test_set_solid_equals_the_models_list_through_set_voxels(H):
    v, t, m = mesh("all")
    want = expected("all", False)
    with make_ctx(H, CFG) as dev, make_ctx(H, CFG) as host:
        dev.set_solid(v, t, m, FILL)
        host.recreate_octree(*want)
        assert_same_scene(dev, host, "set_solid")
        for a, b in zip(dev.get_voxels(), want):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name, shift, grow", [("torus", (0, 0, 0), False), ("icosphere2", (300, 0, 0), True)])
def test_edit_solid_equals_the_models_list_through_edit_voxels(H, scenes, name, shift, grow):
    pos, mrgb, size = scenes.load_scene("menger")
    v, t, m = mesh(name)
    v = (np.rint(v.astype(np.float64) * 16) / 16 + np.array(shift)).astype(np.float32)      # on the snapping grid, so the shift is exact
    want = S.solid(v, t, m, FILL)
    with make_ctx(H, CFG) as dev, make_ctx(H, CFG) as host:
        for c in (dev, host):
            c.recreate_octree(pos, mrgb)
        depth = dev.scene_depth
        if grow:
            with pytest.raises(H.VxrtError) as e:
                dev.edit_solid(v, t, m, FILL)               # outside the root cube without grow
            assert e.value.status == H.E_SCENE
            assert_same_scene(dev, host, "edit_solid refused")
        dev.edit_solid(v, t, m, FILL, grow=grow)
        host.edit_voxels(*want, grow=grow)
        assert (dev.scene_depth > depth) == grow and dev.scene_depth == host.scene_depth
        assert_same_scene(dev, host, f"edit_solid {name}")
        for a, b in zip(dev.get_voxels(), host.get_voxels()):
            assert np.array_equal(a, b)


def test_carve_solid_equals_the_models_list_through_clear_voxels(H, scenes):
    pos, mrgb, size = scenes.load_scene("menger")
    v, t = S.torus(major=20.0, minor=7.0, centre=(40.5, 40.5, 40.5))      # inside the sponge (81^3 cells from 0)
    want = S.solid(v, t, None, FILL, interior_only=True)[0]
    with make_ctx(H, CFG) as dev, make_ctx(H, CFG) as host:
        for c in (dev, host):
            c.recreate_octree(pos, mrgb)
        before = len(dev.get_voxels()[0])
        dev.carve_solid(v, t)
        host.clear_voxels(want)
        assert_same_scene(dev, host, "carve_solid")
        after = dev.get_voxels()[0]
        assert 0 < before - len(after) <= len(want)
        assert not set(map(tuple, after.tolist())) & set(map(tuple, want.tolist()))
