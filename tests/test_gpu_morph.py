"""GPU: vxrt_morph_voxels_device (include/vxrt_morph.h) against its rule in Python (tests/morph_model.py).

Every case compares positions, bytes, order and count with the model for exact equality and checks guard bytes around out_pos and
out_mrgb, that both inputs are unchanged, that a second call writes the same bytes, that the count-only form agrees with and without
a cap, and the wrapper counting first and with room to spare (check: one helper, no lighter mode)."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import morph_model as M
import transform_model as T
from list_op_harness import Bytes, check_call, colours, last_error, on_device

pytestmark = pytest.mark.gpu

MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def raw(ctx, pos, mrgb, n, op, c, steps, out_pos, out_mrgb, cap, count=True):
    """The C call over raw addresses -> (status, *n_out)."""
    torch.cuda.synchronize()
    got = C.c_size_t(0xDEAD)
    rc = ctx._L.vxrt_morph_voxels_device(ctx._h, pos, mrgb, C.c_size_t(n), C.c_uint32(op), C.c_uint32(c), C.c_uint32(steps), out_pos, out_mrgb,
                                         C.c_size_t(cap), C.byref(got) if count else None)
    return rc, got.value


def check(ctx, pos, mrgb, op, c, steps, what, shift=0, want=None):
    """A list, an op, a connectivity and a depth through every form of the call against the model -> (pos, mrgb) of the result.
    want: the model's result, where the caller has it already."""
    what = f"{what}: {M.NAMES[op]} at {c}, {steps} step(s)"
    pos = np.ascontiguousarray(pos, np.int16).reshape(-1, 3)
    mrgb = None if mrgb is None else np.ascontiguousarray(mrgb, np.uint8).reshape(-1, 4)
    want_pos, want_mrgb = M.morph(pos, mrgb, op, c, steps) if want is None else want
    return check_call(ctx, lambda ptr, *out: raw(ctx, *ptr, len(pos), op, c, steps, *out),
                      lambda dev, cap: ctx.morph_voxels(*dev, op, c, steps, cap=cap),
                      [("pos", pos), ("mrgb", mrgb)], want_pos, want_mrgb, what, shift)


def check_ops(ctx, pos, mrgb, c, what, steps=1, shift=0):
    """All four ops -> the results' sizes."""
    return [len(check(ctx, pos, mrgb, op, c, steps, what, shift)[0]) for op in M.OPS]


def cells(*p):
    return np.array(p, np.int16).reshape(-1, 3)


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(32, 32) as c:      # no scene is loaded: the call needs none
        yield c


def random_grid(origin):
    """A 40^3 grid at occupancy 0.3 with its least corner at `origin`, shuffled, 5 % of the cells listed again in other colours."""
    rng = np.random.default_rng(41)
    at = np.argwhere(rng.random((40, 40, 40)) < 0.3)
    at = np.concatenate([at, at[rng.integers(0, len(at), len(at) // 20)]])
    at = at[rng.permutation(len(at))]
    return (at + np.asarray(origin)).astype(np.int16), rng.integers(0, 256, (len(at), 4)).astype(np.uint8)


# ---- the smallest cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.CONNECTIVITIES)
def test_one_voxel_and_nothing(H, ctx, c):
    one, red = cells((3, -4, 5)), np.array([[0x85, 1, 2, 3]], np.uint8)
    assert check_ops(ctx, one, red, c, "one voxel") == [c + 1, 0, 1, c]
    assert check(ctx, one, red, M.SURFACE, c, 1, "bit 7 goes")[1].tolist() == [[5, 1, 2, 3]]
    assert set(map(tuple, check(ctx, one, red, M.MARGIN, c, 1, "the source's bytes")[1].tolist())) == {(5, 1, 2, 3)}
    assert check_ops(ctx, one[:0], red[:0], c, "nothing") == [0, 0, 0, 0]
    # an empty list touches no device pointer
    for op in M.OPS:
        assert raw(ctx, C.c_void_p(8), C.c_void_p(3), 0, op, c, 1, C.c_void_p(5), C.c_void_p(7), 4) == (0, 0)
    assert raw(ctx, None, None, 0, M.MARGIN, c, 64, None, None, 0) == (0, 0)


@pytest.mark.parametrize("c", M.CONNECTIVITIES)
def test_one_voxel_at_each_corner_of_the_int16_range(H, ctx, c):
    inside = {6: 4, 18: 7, 26: 8}[c]                      # the corner and its neighbours that exist: nothing wraps
    n = 0
    for x in (-32768, 32767):
        for y in (-32768, 32767):
            for z in (-32768, 32767):
                n += 1
                assert check_ops(ctx, cells((x, y, z)), colours(1, n), c, f"the corner ({x}, {y}, {z})") == [inside, 0, 1, inside - 1]
    corners = cells(*[(x, y, z) for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)])
    assert check_ops(ctx, corners, colours(8, 9), c, "all eight corners", steps=2)[0] == 8 * {6: 10, 18: 23, 26: 27}[c]


@pytest.mark.parametrize("c", M.CONNECTIVITIES)
def test_two_voxels(H, ctx, c):
    two = colours(2, 10)
    sizes = {}
    for name, other in (("a face", (1, 0, 0)), ("an edge", (1, 1, 0)), ("a corner", (1, 1, 1)), ("two cells apart", (2, 0, 0))):
        sizes[name] = check_ops(ctx, cells((0, 0, 0), other), two, c, "two voxels sharing " + name)
        check_ops(ctx, cells(other, (0, 0, 0)), two, c, "... listed the other way round")
    assert sizes["a face"][0] == {6: 12, 18: 28, 26: 36}[c] and sizes["two cells apart"][0] == {6: 13, 18: 33, 26: 45}[c]
    assert check_ops(ctx, cells((-1, -1, -1), (0, 0, 0)), two, c, "two voxels across the origin")[2] == 2
    # both claim the cell between them: (-1, 0, 0) is row 0, so the voxel at lower x colours it
    got = check(ctx, cells((2, 0, 0), (0, 0, 0)), two, M.DILATE, c, 1, "the cell between")
    assert got[1][got[0].tolist().index([1, 0, 0])].tolist() == [two[1][0] & 0x7F, *two[1][1:]]
    # a red face neighbour comes before a blue edge neighbour
    pair, bytes_ = cells((1, 0, 0), (-1, -1, 0)), np.array([[1, 255, 0, 0], [2, 0, 0, 255]], np.uint8)
    got = check(ctx, pair, bytes_, M.MARGIN, c, 1, "red face, blue edge")
    assert got[1][got[0].tolist().index([0, 0, 0])].tolist() == [1, 255, 0, 0]


def test_one_position_in_four_colours(H, ctx):
    pos = cells(*[(1, 2, 3)] * 4)
    mrgb = np.array([[0x81, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [0xFF, 4, 5, 6]], np.uint8)
    for c in M.CONNECTIVITIES:
        assert check_ops(ctx, pos, mrgb, c, "four colours") == [c + 1, 0, 1, c]
        assert set(map(tuple, check(ctx, pos, mrgb, M.DILATE, c, 1, "the last entry wins")[1].tolist())) == {(0x7F, 4, 5, 6)}


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", M.CONNECTIVITIES)
def test_the_solid_cube_and_the_shell(H, ctx, c):
    cube = M.cube16()
    assert check_ops(ctx, *cube, c, "cube16") == [{6: 5632, 18: 5824, 26: 5832}[c], 2744, 1352, {6: 1536, 18: 1728, 26: 1736}[c]]
    shell = T.shell()
    sizes = check_ops(ctx, *shell, c, "the shell")
    assert sizes[1] == 0 and sizes[2] == len(shell[0])                 # one cell thick: all of it is surface


@pytest.mark.parametrize("c", M.CONNECTIVITIES)
def test_a_plate_of_two_tiles(H, ctx, c):
    # 64 x 64 x 1 = 4 096 voxels, two tiles of the mask kernel: neighbours are found inside the tile, outside it and nowhere
    g = np.arange(-32, 32)
    plate = np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    rng = np.random.default_rng(12)
    order = rng.permutation(len(plate))
    sizes = check_ops(ctx, plate[order], colours(len(plate), 13), c, "the plate")
    assert sizes[1] == 0 and sizes[0] == 4096 + sizes[3]
    flat = np.stack(np.meshgrid(g, [0], g, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    check(ctx, flat, colours(len(flat), 14), M.DILATE, c, 1, "the plate in the x z plane")


@pytest.mark.parametrize("n", [2047, 2048, 2049])
def test_runs_along_x_on_either_side_of_a_tile(H, ctx, n):
    run = np.stack([np.arange(n) - 1000, np.full(n, 7), np.full(n, -3)], -1).astype(np.int16)
    for c in M.CONNECTIVITIES:
        assert check_ops(ctx, run, colours(n, n), c, f"a run of {n}") == [n + {6: 4 * n + 2, 18: 8 * n + 10, 26: 8 * n + 18}[c], 0, n, {6: 4 * n + 2, 18: 8 * n + 10, 26: 8 * n + 18}[c]]


@pytest.mark.parametrize("origin", [(-20, -20, -20), (32728, 32728, 32728)], ids=["around the origin", "ending at 32767"])
@pytest.mark.parametrize("c", M.CONNECTIVITIES)
def test_a_random_grid(H, ctx, c, origin):
    pos, mrgb = random_grid(origin)
    sizes = check_ops(ctx, pos, mrgb, c, "the random grid")
    distinct = len(T.source_of(pos))
    assert len(pos) > distinct > 15000 and sizes[1] + sizes[2] == distinct and sizes[0] == distinct + sizes[3]


@pytest.mark.parametrize("steps", [2, 3])
def test_more_than_one_step(H, ctx, steps):
    rng = np.random.default_rng(15)
    pts = rng.integers(-7, 9, (2500, 3)).astype(np.int16)                 # dense enough to have an inside
    for c in M.CONNECTIVITIES:
        sizes = check_ops(ctx, pts, colours(2500, 16), c, "random points of 16^3", steps=steps)
        assert sizes[0] > len(T.source_of(pts)) > sizes[1]
    assert check_ops(ctx, *M.cube16(), 6, "cube16", steps=steps)[1] == (16 - 2 * steps) ** 3


def test_erode_until_nothing_is_left(H, ctx):
    cube = M.cube16()
    assert len(check(ctx, *cube, M.ERODE, 26, 7, "cube16")[0]) == 8
    for steps in (8, 9, 64):
        assert len(check(ctx, *cube, M.ERODE, 6, steps, "cube16")[0]) == 0
        assert len(check(ctx, *cube, M.SURFACE, 18, steps, "cube16")[0]) == 4096


def test_results_of_0_and_255_to_257_voxels(H, ctx):
    for k in (0, 1, 255, 256, 257):
        # a bar of 3 x 3 x (k + 2): its axis without the two ends survives
        bar = np.array([[x, y, z] for x in (-1, 0, 1) for y in (4, 5, 6) for z in range(-100, -98 + k)], np.int16)
        for c in (6, 26):
            got = check(ctx, bar, colours(len(bar), k), M.ERODE, c, 1, f"a bar that erodes to {k}")
            assert got[0].tolist() == sorted(([0, 5, z] for z in range(-99, -99 + k)), key=T.path_key)
    one = cells((9, 9, 9))
    assert len(check(ctx, np.concatenate([one, one + (3, 0, 0), one + (0, 40, 0)]), colours(3, 17), M.MARGIN, 26, 1, "three specks")[0]) == 78


def test_the_tile_lookup_gives_the_same_bytes(H, ctx):
    # morph_mask_kernel<true> (vxrt_debug.h: the lookup that asks the block's LDS tile first) is kept for measurements: the same
    # cases through it, where neighbours are found inside the tile, outside it and nowhere
    g = np.arange(-32, 32)
    plate = np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    run = np.stack([np.arange(2049) - 1000, np.full(2049, 7), np.full(2049, -3)], -1).astype(np.int16)
    assert ctx._L.vxrt_debug_morph_tile_lookup(ctx._h, C.c_uint32(1)) == 0
    try:
        for c in M.CONNECTIVITIES:
            check_ops(ctx, plate, colours(len(plate), 13), c, "the plate, tile lookup")
            check_ops(ctx, run, colours(2049, 22), c, "a run of 2 049, tile lookup")
        check_ops(ctx, *random_grid((32728, -20, -32768)), 26, "the random grid, tile lookup")
        check_ops(ctx, *M.cube16(), 18, "cube16, tile lookup", steps=2)
    finally:
        assert ctx._L.vxrt_debug_morph_tile_lookup(ctx._h, C.c_uint32(0)) == 0
    assert ctx._L.vxrt_debug_morph_tile_lookup(None, C.c_uint32(1)) == H.E_INVALID


# ---- addresses, values, room -------------------------------------------------------------------------------------------------------
def test_all_arrays_at_odd_addresses(H, ctx):
    rng = np.random.default_rng(18)
    pts = rng.integers(-6, 6, (900, 3)).astype(np.int16)
    for shift in (1, 2, 3, 7):
        for op in M.OPS:
            check(ctx, pts, colours(900, 19), op, 18, 1, f"addresses = {shift} mod 16", shift=shift)
    check(ctx, pts, None, M.DILATE, 26, 2, "positions only at an odd address", shift=5)


def test_positions_only(H, ctx):
    rng = np.random.default_rng(20)
    pts = rng.integers(-6, 6, (900, 3)).astype(np.int16)
    for op in M.OPS:
        for c in M.CONNECTIVITIES:
            only = check(ctx, pts, None, op, c, 1, "positions only")
            full = check(ctx, pts, colours(900, 21), op, c, 1, "with bytes")
            assert only[1] is None and np.array_equal(only[0], full[0])


def test_room_for_exactly_the_count_and_for_one_less(H, ctx):
    pos, mrgb = M.cube16()
    want = M.morph(pos, mrgb, M.DILATE, 18, 1)
    k = len(want[0])
    dev = [on_device(pos), on_device(mrgb)]
    args = (ctx, C.c_void_p(dev[0].data_ptr()), C.c_void_p(dev[1].data_ptr()), len(pos), M.DILATE, 18, 1)
    out_pos, out_mrgb = Bytes(6 * k), Bytes(4 * k)
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, k - 1) == (H.E_INVALID, k)
    assert str(k) in last_error(ctx) and str(k - 1) in last_error(ctx) and "vxrt_morph_voxels_device" in last_error(ctx)
    assert out_pos.untouched() and out_mrgb.untouched()
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, 0) == (H.E_INVALID, k) and out_pos.untouched() and out_mrgb.untouched()
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, k) == (0, k) and out_pos.guards_hold() and out_mrgb.guards_hold()
    assert np.array_equal(out_pos.data().view(np.int16).reshape(-1, 3), want[0]) and np.array_equal(out_mrgb.data().reshape(-1, 4), want[1])
    with pytest.raises(H.VxrtError) as e:
        ctx.morph_voxels(*dev, H.MORPH_DILATE, 18, 1, cap=k - 1)
    assert e.value.status == H.E_INVALID


def test_the_outputs_may_be_the_inputs_arrays(H, ctx):
    rng = np.random.default_rng(30)
    pos, mrgb = M.cube16()
    order = rng.permutation(len(pos))
    pos, mrgb = pos[order], mrgb[order]
    for op, steps in ((M.ERODE, 1), (M.SURFACE, 2)):
        want = M.morph(pos, mrgb, op, 6, steps)
        k = len(want[0])
        assert 0 < k < len(pos)
        io_pos, io_mrgb = Bytes(6 * len(pos), 0, pos), Bytes(4 * len(pos), 0, mrgb)
        assert raw(ctx, io_pos.ptr, io_mrgb.ptr, len(pos), op, 6, steps, io_pos.ptr, io_mrgb.ptr, len(pos)) == (0, k), last_error(ctx)
        assert io_pos.guards_hold() and io_mrgb.guards_hold()
        assert np.array_equal(io_pos.data()[:6 * k].view(np.int16).reshape(-1, 3), want[0]) and np.array_equal(io_mrgb.data()[:4 * k].reshape(-1, 4), want[1])
        # behind the result the input's bytes stand as they were
        assert io_pos.data()[6 * k:].tobytes() == pos.tobytes()[6 * k:] and io_mrgb.data()[4 * k:].tobytes() == mrgb.tobytes()[4 * k:]


def test_refusals_write_nothing(H, ctx):
    pos, mrgb = M.cube16()
    n = len(pos)
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    p, c = C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr())
    out_pos, out_mrgb = Bytes(6 * 2 * n), Bytes(4 * 2 * n)
    o, w, room = out_pos.ptr, out_mrgb.ptr, 2 * n

    def refused(*args, status=H.E_INVALID, says=None, **kw):
        assert raw(ctx, *args, **kw) == (status, 0xDEAD), args
        assert last_error(ctx) and (says is None or says in last_error(ctx)), last_error(ctx)
        assert out_pos.untouched() and out_mrgb.untouched()

    refused(p, c, 1 << 32, M.DILATE, 6, 1, o, w, room, says="2^32")                    # before any pointer is looked at
    refused(None, None, 1 << 32, 9, 5, 0, None, None, 0, says="2^32", count=False)
    refused(p, c, n, M.DILATE, 6, 1, o, w, room, says="n_out", count=False)
    for op in (4, 5, 0xFFFFFFFF):
        refused(p, c, n, op, 6, 1, o, w, room, says="vxrt_morph_op")
    for conn in (0, 4, 8, 27, 0xFFFFFFFF):
        refused(p, c, n, M.ERODE, conn, 1, o, w, room, says="connectivity")
    for steps in (0, 65, 0xFFFFFFFF):
        refused(p, c, n, M.ERODE, 6, steps, o, w, room, says="steps")
    refused(p, c, n, 4, 7, 0, o, w, room, says="vxrt_morph_op")                        # in the header's order
    refused(p, c, n, M.MARGIN, 7, 0, o, w, room, says="connectivity")
    for op in M.OPS:
        refused(p, c, n, op, 6, 1, o, None, room, says="both or neither")
        refused(p, c, n, op, 6, 1, None, w, room, says="both or neither")
        refused(p, None, n, op, 6, 1, o, w, room, says="out_mrgb without mrgb")
        refused(p, None, n, op, 6, 1, None, w, room, says="out_mrgb without mrgb")
    refused(None, c, n, M.DILATE, 6, 1, o, w, room, says="null voxel positions")
    # host memory, pageable and pinned
    refused(C.c_void_p(pos.ctypes.data), c, n, M.DILATE, 6, 1, o, w, room, says="pos")
    assert "not device memory" in last_error(ctx)
    pinned = torch.as_tensor(np.array(mrgb)).pin_memory()
    refused(p, C.c_void_p(pinned.data_ptr()), n, M.DILATE, 6, 1, o, w, room, says="mrgb")
    host_pos, host_mrgb = np.zeros((room, 3), np.int16), np.zeros((room, 4), np.uint8)
    refused(p, c, n, M.DILATE, 6, 1, C.c_void_p(host_pos.ctypes.data), w, room, says="out_pos")
    refused(p, c, n, M.DILATE, 6, 1, o, C.c_void_p(host_mrgb.ctypes.data), room, says="out_mrgb")
    assert not host_pos.any() and not host_mrgb.any()
    # an output one entry short of its cap: an allocation of its own, because what the library can see is the allocation
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    cap = 1025                                                                      # 1024 entries of 4 bytes are a whole page: no rounding hides the missing one
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (cap - 1))) == 0
    refused(p, c, n, M.ERODE, 6, 7, o, short, cap, says="past its allocation")
    assert "out_mrgb" in last_error(ctx)
    assert hip.hipFree(short) == 0
    # ... and the valid call is accepted afterwards
    assert raw(ctx, p, c, n, M.ERODE, 6, 1, o, w, room) == (0, 2744) and out_pos.guards_hold() and out_mrgb.guards_hold()
    assert np.array_equal(d_pos.cpu().numpy(), pos) and np.array_equal(d_mrgb.cpu().numpy(), mrgb)


# ---- beside the rest of the library ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cube16", "the random grid"])
def test_surface_and_margin_are_what_combine_voxels_gives(H, ctx, which):
    pos, mrgb = M.cube16() if which == "cube16" else random_grid((-20, -20, -20))
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    for c in M.CONNECTIVITIES:
        for steps in (1, 2):
            eroded = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_ERODE, c, steps)
            surface = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_SURFACE, c, steps)
            want = ctx.combine_voxels(d_pos, d_mrgb, eroded[0], None, H.LIST_DIFFERENCE)
            assert len(surface[0]) > 0 and torch.equal(surface[0], want[0]) and torch.equal(surface[1], want[1]), (c, steps)
            dilated = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_DILATE, c, steps)
            margin = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_MARGIN, c, steps)
            want = ctx.combine_voxels(*dilated, d_pos, None, H.LIST_DIFFERENCE)
            assert len(margin[0]) > 0 and torch.equal(margin[0], want[0]) and torch.equal(margin[1], want[1]), (c, steps)
    # dilation joins components and never splits one
    _, before = ctx.label_components(d_pos, 26)
    _, after = ctx.label_components(ctx.morph_voxels(d_pos, None, H.MORPH_DILATE, 26)[0], 26)
    assert 1 <= after <= before
    # closing fills what opening never makes: both stay within one dilation of the set
    closed, opened = ctx.close_voxels(d_pos, d_mrgb, 6), ctx.open_voxels(d_pos, d_mrgb, 6)
    src = T.source_of(pos, mrgb)
    want_closed = M.morph(*M.morph(pos, mrgb, M.DILATE, 6), M.ERODE, 6)
    assert np.array_equal(closed[0].cpu().numpy(), want_closed[0]) and np.array_equal(closed[1].cpu().numpy(), want_closed[1])
    closed_cells = {tuple(q) for q in want_closed[0].tolist()}
    assert all(tuple(p) in src for p in opened[0].cpu().numpy().tolist()) and all(p in closed_cells for p in src)


def test_the_scorch_ring_of_a_crater_in_the_sponge(H):
    with H.Context(32, 32) as c:
        c.set_menger(3, 0, MENGER_MRGB)
        before = c.get_voxels_device()
        assert len(before[0]) == 8000
        pos = before[0].cpu().numpy().astype(np.int64)
        lo = pos.min(axis=0)
        g = np.arange(-6, 7)                                                 # around lo + 20, in a solid corner: the sponge's own centre is a hole
        ball = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        ball = (ball[(ball ** 2).sum(axis=1) < 5.5 ** 2] + lo + 20).astype(np.int16)      # H: cells of the ball, voxels or not
        scene = {tuple(p): tuple(b) for p, b in zip(pos.tolist(), before[1].cpu().numpy().tolist())}
        assert any(tuple(p) in scene for p in ball.tolist())
        # 1. the crater
        d_ball = on_device(ball)
        c.clear_voxels_device(d_ball)
        # 2. the ring around it, where the scene has voxels
        ring, _ = c.morph_voxels(d_ball, None, H.MORPH_MARGIN, 26)
        hit, _ = c.combine_voxels(ring, None, *c.get_voxels_device()[:1], None, H.LIST_INTERSECT)
        assert 0 < len(hit) < len(ring)
        # 3. scorched
        soot = (3, 20, 20, 20)
        c.edit_voxels_device(hit, on_device(np.tile(np.array([soot], np.uint8), (len(hit), 1))))
        # 4. the same on a dict
        for p in ball.tolist():
            scene.pop(tuple(p), None)
        for p in M.morph(ball, None, M.MARGIN, 26)[0].tolist():
            if tuple(p) in scene:
                scene[tuple(p)] = soot
        got = c.get_voxels_device()
        order = sorted(scene, key=T.path_key)
        assert got[0].cpu().numpy().tolist() == [list(p) for p in order] and got[1].cpu().numpy().tolist() == [list(scene[p]) for p in order]
        assert sum(1 for b in scene.values() if b == soot) == len(hit)
