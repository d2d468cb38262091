"""GPU: vxrt_distance_voxels_device (include/vxrt_distance.h) against its rule in Python (tests/distance_model.py).

Every case compares positions, bytes, d2, order and count with the model for exact equality and checks guard bytes around out_pos,
out_mrgb and out_d2, that both inputs are unchanged, that a second call writes the same bytes, that the count-only form agrees with
and without a cap, and the wrapper counting first and with room to spare (check: one helper, no lighter mode)."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import distance_model as D
import morph_model as M
import transform_model as T
from list_op_harness import DEV, Bytes, colours, last_error, on_device
from test_distance_cpu import BLUE, GREEN, RANGE_CORNERS, RED, tie_cases, tile_corner_voxels

pytestmark = pytest.mark.gpu

MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)
NAME = "vxrt_distance_voxels_device"


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def raw(ctx, pos, mrgb, n, mode, max_d2, out_pos, out_mrgb, out_d2, cap, count=True):
    """The C call over raw addresses -> (status, *n_out)."""
    torch.cuda.synchronize()
    got = C.c_size_t(0xDEAD)
    rc = ctx._L.vxrt_distance_voxels_device(ctx._h, pos, mrgb, C.c_size_t(n), C.c_uint32(mode), C.c_uint32(max_d2), out_pos, out_mrgb, out_d2,
                                            C.c_size_t(cap), C.byref(got) if count else None)
    return rc, got.value


_WANT = {}


def model(pos, mrgb, mode, max_d2):
    """distance_model.distance_np, computed once per list, mode and radius and never changed."""
    key = (pos.tobytes(), None if mrgb is None else mrgb.tobytes(), mode, max_d2)
    if key not in _WANT:
        _WANT[key] = D.distance_np(pos, mrgb, mode, max_d2)
        for a in _WANT[key]:
            if a is not None:
                a.setflags(write=False)
    return _WANT[key]


def check(ctx, pos, mrgb, mode, max_d2, what, shift=0):
    """A list, a mode and a squared radius through every form of the call against the model -> (pos, mrgb, d2) of the result."""
    what = f"{what}: {D.NAMES[mode]} at max_d2 {max_d2}"
    pos = np.ascontiguousarray(pos, np.int16).reshape(-1, 3)
    mrgb = None if mrgb is None else np.ascontiguousarray(mrgb, np.uint8).reshape(-1, 4)
    want_pos, want_mrgb, want_d2 = model(pos, mrgb, mode, max_d2)
    with_vals = mrgb is not None
    k, n = len(want_pos), len(pos)
    ins = [Bytes(pos.nbytes, shift, pos), Bytes(mrgb.nbytes, shift, mrgb) if with_vals else None]
    ptr = [None if b is None else b.ptr for b in ins]
    if n == 0 and with_vals:
        ptr[1] = C.c_void_p(3)                 # "bytes, and no entries": an address that is never read
    args = (ctx, *ptr, n, mode, max_d2)
    assert raw(*args, None, None, None, 0) == (0, k), (what, "count only", last_error(ctx))
    assert raw(*args, None, None, None, 12345) == (0, k), (what, "count only ignores cap")
    outs = []
    for turn in range(2):
        out = [Bytes(6 * k, shift), Bytes(4 * k, shift) if with_vals else None, Bytes(2 * k, shift)]
        assert raw(*args, *[None if b is None else b.ptr for b in out], k) == (0, k), (what, f"call {turn}", last_error(ctx))
        assert all(b is None or b.guards_hold() for b in out), f"{what}: guard bytes"
        outs.append(out)
    got_pos = outs[0][0].data().view(np.int16).reshape(-1, 3)
    assert np.array_equal(got_pos, want_pos), f"{what}: {int((got_pos != want_pos).any(axis=1).sum())} of {k} positions differ"
    got_d2 = outs[0][2].data().view(np.uint16)
    assert np.array_equal(got_d2, want_d2), f"{what}: {int((got_d2 != want_d2).sum())} of {k} d2 differ"
    got_mrgb = None
    if with_vals:
        got_mrgb = outs[0][1].data().reshape(-1, 4)
        assert np.array_equal(got_mrgb, want_mrgb), f"{what}: {int((got_mrgb != want_mrgb).any(axis=1).sum())} of {k} voxels' bytes differ"
    for a, b in zip(*outs):
        assert a is None or a.all().tobytes() == b.all().tobytes(), f"{what}: a second call"
    for b, (name, v) in zip(ins, (("pos", pos), ("mrgb", mrgb))):
        assert b is None or (b.guards_hold() and b.data().tobytes() == v.tobytes()), f"{what}: {name} was written"
    # the wrapper, counting first and with room to spare
    dev = [on_device(pos), on_device(mrgb) if with_vals else None]
    for cap in (None, k + 3):
        w_pos, w_mrgb, w_d2 = ctx.distance_voxels(*dev, mode, max_d2, cap=cap)
        assert w_pos.dtype == torch.int16 and w_pos.device == DEV and tuple(w_pos.shape) == (k, 3), what
        assert w_d2.dtype == torch.uint16 and w_d2.device == DEV and tuple(w_d2.shape) == (k,), what
        assert np.array_equal(w_pos.cpu().numpy(), want_pos) and np.array_equal(w_d2.cpu().numpy(), want_d2), f"{what}: the wrapper"
        assert (w_mrgb is None) == (not with_vals)
        if with_vals:
            assert w_mrgb.dtype == torch.uint8 and tuple(w_mrgb.shape) == (k, 4) and np.array_equal(w_mrgb.cpu().numpy(), want_mrgb), f"{what}: the wrapper"
    return got_pos, got_mrgb, got_d2


def check_modes(ctx, pos, mrgb, max_d2, what, shift=0):
    """All four modes -> the results' sizes."""
    return [len(check(ctx, pos, mrgb, mode, max_d2, what, shift)[0]) for mode in D.MODES]


def cells(*p):
    return np.array(p, np.int16).reshape(-1, 3)


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(32, 32) as c:      # no scene is loaded: the call needs none
        yield c


def random_grid(origin, occupancy):
    """A 40^3 grid at an occupancy with its least corner at `origin`, shuffled, 5 % of the cells listed again in other colours."""
    rng = np.random.default_rng(43)
    at = np.argwhere(rng.random((40, 40, 40)) < occupancy)
    at = np.concatenate([at, at[rng.integers(0, len(at), max(1, len(at) // 20))]])
    at = at[rng.permutation(len(at))]
    return (at + np.asarray(origin)).astype(np.int16), rng.integers(0, 256, (len(at), 4)).astype(np.uint8)


BALL = {1: 7, 2: 19, 3: 27, 4: 33, 255: 17071, 256: 17077}


# ---- the smallest cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_d2", sorted(BALL))
def test_one_voxel_and_nothing(H, ctx, max_d2):
    one, red = cells((3, -4, 5)), np.array([[0x85, 1, 2, 3]], np.uint8)
    assert check_modes(ctx, one, red, max_d2, "one voxel") == [1, BALL[max_d2] - 1, 0, BALL[max_d2]]
    got = check(ctx, one, red, D.DEPTH, max_d2, "bit 7 goes")
    assert got[1].tolist() == [[5, 1, 2, 3]] and got[2].tolist() == [1]
    got = check(ctx, one, red, D.FIELD, max_d2, "the source's bytes")
    assert set(map(tuple, got[1].tolist())) == {(5, 1, 2, 3)} and int(got[2].max()) == max(d for d in (1, 2, 3, 4, 254, 256) if d <= max_d2)
    assert check_modes(ctx, one[:0], red[:0], max_d2, "nothing") == [0, 0, 0, 0]
    assert check_modes(ctx, one[:0], None, max_d2, "nothing, positions only") == [0, 0, 0, 0]
    # an empty list touches no device pointer
    for mode in D.MODES:
        assert raw(ctx, C.c_void_p(8), C.c_void_p(3), 0, mode, max_d2, C.c_void_p(5), C.c_void_p(7), C.c_void_p(9), 4) == (0, 0)
    assert raw(ctx, None, None, 0, D.FIELD, max_d2, None, None, None, 0) == (0, 0)


def test_one_voxel_at_each_corner_of_a_tile(H, ctx):
    for n, one in enumerate(tile_corner_voxels()):
        for max_d2 in (1, 3, 256):
            assert check_modes(ctx, one, colours(1, n), max_d2, f"the voxel {one.tolist()}") == [1, BALL[max_d2] - 1, 0, BALL[max_d2]]


def test_the_corners_of_the_int16_range(H, ctx):
    for n, corner in enumerate(RANGE_CORNERS):
        one = corner.reshape(1, 3)
        assert check_modes(ctx, one, colours(1, 20 + n), 3, f"the corner {corner.tolist()}") == [1, 7, 0, 8]      # nothing wraps
        assert check(ctx, one, None, D.DEPTH, 256, "a voxel on the edge of the range has depth 1")[2].tolist() == [1]
    sizes = check_modes(ctx, RANGE_CORNERS, colours(8, 30), 256, "all eight corners")
    assert sizes[0] == 8 and sizes[2] == 0 and sizes[3] == sizes[1] + 8


def test_the_ties_in_colour(H, ctx):
    for pos, mrgb, max_d2, cell, want in tie_cases():
        for order in (np.arange(len(pos)), np.arange(len(pos))[::-1]):
            for mode in (D.FIELD, D.DILATE):
                got = check(ctx, pos[order], mrgb[order], mode, max_d2, f"the tie {pos.tolist()}")
                assert got[1][got[0].tolist().index(list(cell))].tolist() == list(want)
    assert {RED, BLUE, GREEN} == {want for *_, want in tie_cases()}


def test_two_voxels_whose_fields_just_meet(H, ctx):
    two = colours(2, 40)
    apart = check(ctx, cells((0, 0, 0), (33, 0, 0)), two, D.FIELD, 256, "33 apart")
    assert len(apart[0]) == 2 * (BALL[256] - 1)                          # |dx| <= 16 from each: 16 and 17 do not meet
    meet = check(ctx, cells((0, 0, 0), (32, 0, 0)), two, D.FIELD, 256, "32 apart")
    assert len(meet[0]) == 2 * (BALL[256] - 1) - 1                       # (16, 0, 0) is both balls' pole ...
    assert meet[1][meet[0].tolist().index([16, 0, 0])].tolist() == [two[0][0] & 0x7F, *two[0][1:]]      # ... and takes the voxel at -x
    check_modes(ctx, cells((32, 0, 0), (0, 0, 0)), two, 255, "32 apart at 255")


def test_one_position_in_four_colours(H, ctx):
    pos = cells(*[(1, 2, 3)] * 4)
    mrgb = np.array([[0x81, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [0xFF, 4, 5, 6]], np.uint8)
    for max_d2 in (1, 5):
        assert check_modes(ctx, pos, mrgb, max_d2, "four colours") == [1, len(D.offsets(max_d2)) - 1, 0, len(D.offsets(max_d2))]
        assert set(map(tuple, check(ctx, pos, mrgb, D.DILATE, max_d2, "the last entry wins")[1].tolist())) == {(0x7F, 4, 5, 6)}


# ---- shapes ------------------------------------------------------------------------------------------------------------------------
def test_cube16(H, ctx):
    cube = M.cube16()
    assert [len(check(ctx, *cube, D.ERODE, m, "cube16")[0]) for m in (1, 3, 4, 49, 63, 64)] == [2744, 2744, 1728, 8, 8, 0]
    assert check_modes(ctx, *cube, 4, "cube16") == [4096, 3272, 1728, 7368]
    check(ctx, *cube, D.DEPTH, 64, "cube16")
    check(ctx, *cube, D.DILATE, 9, "cube16")


def test_the_solid_31(H, ctx):
    c31 = D.solid(31, -15)
    assert [len(check(ctx, *c31, D.ERODE, m, "the solid 31^3")[0]) for m in (255, 256)] == [1, 0]


def test_the_solid_33(H, ctx):
    c33 = D.solid(33, -16)
    got = check(ctx, *c33, D.ERODE, 256, "the solid 33^3")
    assert got[0].tolist() == [[0, 0, 0]] and got[2].tolist() == [D.FAR]
    got = check(ctx, *c33, D.DEPTH, 256, "the solid 33^3")
    assert got[2][got[0].tolist().index([0, 0, 0])] == D.FAR and int((got[2] == D.FAR).sum()) == 1
    check(ctx, *c33, D.DILATE, 2, "the solid 33^3")


def test_the_shell_of_cube16(H, ctx):
    shell = T.shell()
    sizes = check_modes(ctx, *shell, 5, "the shell")
    assert sizes[0] == len(shell[0]) and sizes[2] == 0                  # one cell thick: nothing is deep
    inside = check(ctx, *shell, D.FIELD, 64, "the shell")               # the hollow fills from the walls: its centre is 8 away
    assert [0, 0, 0] in inside[0].tolist() and inside[2][inside[0].tolist().index([0, 0, 0])] == 64


def test_a_plate_and_a_run(H, ctx):
    # 64 x 64 x 1 = 4 096 voxels over 16 tiles; 2 049 voxels along x over 129
    g = np.arange(-32, 32)
    plate = np.stack(np.meshgrid(g, g, [0], indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    order = np.random.default_rng(12).permutation(len(plate))
    sizes = check_modes(ctx, plate[order], colours(len(plate), 13), 9, "the plate")
    assert sizes[0] == 4096 and sizes[2] == 0 and sizes[3] == 4096 + sizes[1]
    flat = np.stack(np.meshgrid(g, [0], g, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
    check(ctx, flat, colours(len(flat), 14), D.DILATE, 2, "the plate in the x z plane")
    n = 2049
    run = np.stack([np.arange(n) - 1000, np.full(n, 7), np.full(n, -3)], -1).astype(np.int16)
    assert check_modes(ctx, run, colours(n, n), 2, f"a run of {n}") == [n, 8 * n + 10, 0, 9 * n + 10]
    check(ctx, run, colours(n, n), D.FIELD, 20, f"a run of {n}")


@pytest.mark.parametrize("origin", [(-20, -20, -20), (32728, 32728, 32728)], ids=["around the origin", "ending at 32767"])
def test_a_dense_random_grid(H, ctx, origin):
    pos, mrgb = random_grid(origin, 0.3)
    distinct = len(T.source_of(pos))
    assert len(pos) > distinct > 15000
    for max_d2 in (1, 6):
        sizes = check_modes(ctx, pos, mrgb, max_d2, "the random grid")
        assert sizes[0] == distinct and sizes[3] == distinct + sizes[1]
    assert 0 < len(check(ctx, pos, mrgb, D.ERODE, 1, "the random grid")[0]) < 100          # all six neighbours set: rare


@pytest.mark.parametrize("origin", [(-20, -20, -20), (32728, 32728, 32728)], ids=["around the origin", "ending at 32767"])
def test_a_sparse_random_grid(H, ctx, origin):
    pos, mrgb = random_grid(origin, 0.002)
    distinct = len(T.source_of(pos))
    assert len(pos) > distinct > 80
    for max_d2 in (20, 256):                                                                # long distances, through many tiles
        sizes = check_modes(ctx, pos, mrgb, max_d2, "the sparse grid")
        assert sizes[0] == distinct and sizes[2] == 0 and sizes[3] == distinct + sizes[1]
    # ... and its complement within the box: long distances to the nearest empty cell, and FAR at a small radius
    full = np.stack(np.meshgrid(*[np.arange(40)] * 3, indexing="ij"), -1).reshape(-1, 3) + np.asarray(origin)
    holes = {tuple(p) for p in pos.tolist()}
    rest = np.array([p for p in full.tolist() if tuple(p) not in holes], np.int16)
    got = check(ctx, rest, None, D.DEPTH, 9, "the box without the sparse grid")
    assert int((got[2] == D.FAR).sum()) > 1000 and int((got[2] == 9).sum()) > 100
    check(ctx, rest, None, D.ERODE, 256, "the box without the sparse grid")


def test_results_of_0_and_255_to_257_voxels(H, ctx):
    for k in (0, 1, 255, 256, 257):
        # a bar of 3 x 3 x (k + 2): its axis without the two ends is deeper than 3
        bar = np.array([[x, y, z] for x in (-1, 0, 1) for y in (4, 5, 6) for z in range(-100, -98 + k)], np.int16)
        got = check(ctx, bar, colours(len(bar), k), D.ERODE, 3, f"a bar that erodes to {k}")
        assert got[0].tolist() == sorted(([0, 5, z] for z in range(-99, -99 + k)), key=T.path_key)


# ---- addresses, values, room -------------------------------------------------------------------------------------------------------
def test_all_arrays_at_odd_addresses(H, ctx):
    rng = np.random.default_rng(18)
    pts = rng.integers(-6, 6, (900, 3)).astype(np.int16)
    for shift in (1, 2, 3, 7):
        for mode in D.MODES:
            check(ctx, pts, colours(900, 19), mode, 5, f"addresses = {shift} mod 16", shift=shift)
    check(ctx, pts, None, D.DILATE, 9, "positions only at an odd address", shift=5)


def test_positions_only_and_without_out_d2(H, ctx):
    rng = np.random.default_rng(20)
    pts = rng.integers(-6, 6, (900, 3)).astype(np.int16)
    bytes_ = colours(900, 21)
    for mode in D.MODES:
        for max_d2 in (2, 10):
            only = check(ctx, pts, None, mode, max_d2, "positions only")
            full = check(ctx, pts, bytes_, mode, max_d2, "with bytes")
            assert only[1] is None and np.array_equal(only[0], full[0]) and np.array_equal(only[2], full[2])
            # out_d2 omitted: the other arrays take the same bytes
            k = len(full[0])
            d_pos, d_mrgb = on_device(pts), on_device(bytes_)
            out_pos, out_mrgb = Bytes(6 * k), Bytes(4 * k)
            assert raw(ctx, C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr()), 900, mode, max_d2, out_pos.ptr, out_mrgb.ptr, None, k) == (0, k)
            assert out_pos.guards_hold() and out_mrgb.guards_hold()
            assert np.array_equal(out_pos.data().view(np.int16).reshape(-1, 3), full[0]) and np.array_equal(out_mrgb.data().reshape(-1, 4), full[1])
            out_pos = Bytes(6 * k)
            assert raw(ctx, C.c_void_p(d_pos.data_ptr()), None, 900, mode, max_d2, out_pos.ptr, None, None, k) == (0, k)
            assert out_pos.guards_hold() and np.array_equal(out_pos.data().view(np.int16).reshape(-1, 3), full[0])


def test_room_for_exactly_the_count_and_for_one_less(H, ctx):
    pos, mrgb = M.cube16()
    want = model(pos, mrgb, D.DILATE, 2)
    k = len(want[0])
    dev = [on_device(pos), on_device(mrgb)]
    args = (ctx, C.c_void_p(dev[0].data_ptr()), C.c_void_p(dev[1].data_ptr()), len(pos), D.DILATE, 2)
    out = [Bytes(6 * k), Bytes(4 * k), Bytes(2 * k)]
    ptrs = [b.ptr for b in out]
    assert raw(*args, *ptrs, k - 1) == (H.E_INVALID, k)
    assert str(k) in last_error(ctx) and str(k - 1) in last_error(ctx) and NAME in last_error(ctx)
    assert all(b.untouched() for b in out)
    assert raw(*args, *ptrs, 0) == (H.E_INVALID, k) and all(b.untouched() for b in out)
    assert raw(*args, *ptrs, k) == (0, k) and all(b.guards_hold() for b in out)
    assert np.array_equal(out[0].data().view(np.int16).reshape(-1, 3), want[0]) and np.array_equal(out[1].data().reshape(-1, 4), want[1])
    assert np.array_equal(out[2].data().view(np.uint16), want[2])
    with pytest.raises(H.VxrtError) as e:
        ctx.distance_voxels(*dev, H.DISTANCE_DILATE, 2, cap=k - 1)
    assert e.value.status == H.E_INVALID


def test_the_outputs_may_be_the_inputs_arrays(H, ctx):
    rng = np.random.default_rng(30)
    pos, mrgb = M.cube16()
    order = rng.permutation(len(pos))
    pos, mrgb = pos[order], mrgb[order]
    for mode, max_d2 in ((D.ERODE, 4), (D.DEPTH, 9)):
        want = model(pos, mrgb, mode, max_d2)
        k = len(want[0])
        assert 0 < k <= len(pos)
        io_pos, io_mrgb, d2 = Bytes(6 * len(pos), 0, pos), Bytes(4 * len(pos), 0, mrgb), Bytes(2 * k)
        assert raw(ctx, io_pos.ptr, io_mrgb.ptr, len(pos), mode, max_d2, io_pos.ptr, io_mrgb.ptr, d2.ptr, len(pos)) == (0, k), last_error(ctx)
        assert io_pos.guards_hold() and io_mrgb.guards_hold() and d2.guards_hold()
        assert np.array_equal(io_pos.data()[:6 * k].view(np.int16).reshape(-1, 3), want[0]) and np.array_equal(io_mrgb.data()[:4 * k].reshape(-1, 4), want[1])
        assert np.array_equal(d2.data().view(np.uint16), want[2])
        # behind the result the input's bytes stand as they were
        assert io_pos.data()[6 * k:].tobytes() == pos.tobytes()[6 * k:] and io_mrgb.data()[4 * k:].tobytes() == mrgb.tobytes()[4 * k:]


def test_refusals_write_nothing(H, ctx):
    pos, mrgb = M.cube16()
    n = len(pos)
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    p, c = C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr())
    out_pos, out_mrgb, out_d2 = Bytes(6 * 2 * n), Bytes(4 * 2 * n), Bytes(2 * 2 * n)
    o, w, d, room = out_pos.ptr, out_mrgb.ptr, out_d2.ptr, 2 * n

    def refused(*args, status=H.E_INVALID, says=None, **kw):
        assert raw(ctx, *args, **kw) == (status, 0xDEAD), args
        assert last_error(ctx) and (says is None or says in last_error(ctx)), last_error(ctx)
        assert out_pos.untouched() and out_mrgb.untouched() and out_d2.untouched()

    refused(p, c, 1 << 32, D.DILATE, 1, o, w, d, room, says="2^32")                     # before any pointer is looked at
    refused(None, None, 1 << 32, 9, 0, None, None, None, 0, says="2^32", count=False)
    refused(p, c, n, D.DILATE, 1, o, w, d, room, says="n_out", count=False)
    for mode in (4, 5, 0xFFFFFFFF):
        refused(p, c, n, mode, 1, o, w, d, room, says="vxrt_distance_mode")
    for max_d2 in (0, 257, 0xFFFFFFFF):
        refused(p, c, n, D.ERODE, max_d2, o, w, d, room, says="max_d2")
    refused(p, c, n, 4, 0, o, w, d, room, says="vxrt_distance_mode")                     # in the header's order
    refused(p, c, n, D.FIELD, 0, o, None, d, room, says="max_d2")
    for mode in D.MODES:
        refused(p, c, n, mode, 4, o, None, d, room, says="both or neither")
        refused(p, c, n, mode, 4, None, w, None, room, says="both or neither")
        refused(p, None, n, mode, 4, o, w, d, room, says="out_mrgb without mrgb")
        refused(p, None, n, mode, 4, None, w, None, room, says="out_mrgb without mrgb")
        refused(p, c, n, mode, 4, None, None, d, room, says="out_d2 without out_pos")
        refused(p, None, n, mode, 4, None, None, d, room, says="out_d2 without out_pos")
    refused(None, c, n, D.DILATE, 4, o, w, d, room, says="null voxel positions")
    # host memory, pageable and pinned
    refused(C.c_void_p(pos.ctypes.data), c, n, D.DILATE, 4, o, w, d, room, says="pos")
    assert "not device memory" in last_error(ctx)
    pinned = torch.as_tensor(np.array(mrgb)).pin_memory()
    refused(p, C.c_void_p(pinned.data_ptr()), n, D.DILATE, 4, o, w, d, room, says="mrgb")
    host_pos, host_mrgb, host_d2 = np.zeros((room, 3), np.int16), np.zeros((room, 4), np.uint8), np.zeros(room, np.uint16)
    refused(p, c, n, D.DILATE, 4, C.c_void_p(host_pos.ctypes.data), w, d, room, says="out_pos")
    refused(p, c, n, D.DILATE, 4, o, C.c_void_p(host_mrgb.ctypes.data), d, room, says="out_mrgb")
    refused(p, c, n, D.DILATE, 4, o, w, C.c_void_p(host_d2.ctypes.data), room, says="out_d2")
    assert not host_pos.any() and not host_mrgb.any() and not host_d2.any()
    # an output one entry short of its cap: an allocation of its own, because what the library can see is the allocation
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    cap = 2049                                                                      # 2048 entries of 2 bytes are a whole page: no rounding hides the missing one
    assert hip.hipMalloc(C.byref(short), C.c_size_t(2 * (cap - 1))) == 0
    refused(p, c, n, D.ERODE, 49, o, w, short, cap, says="past its allocation")
    assert "out_d2" in last_error(ctx)
    assert hip.hipFree(short) == 0
    # ... and the valid call is accepted afterwards
    assert raw(ctx, p, c, n, D.ERODE, 1, o, w, d, room) == (0, 2744) and out_pos.guards_hold() and out_mrgb.guards_hold() and out_d2.guards_hold()
    assert np.array_equal(d_pos.cpu().numpy(), pos) and np.array_equal(d_mrgb.cpu().numpy(), mrgb)


# ---- beside the rest of the library ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["cube16", "the random grid"])
def test_beside_morphology(H, ctx, which):
    pos, mrgb = M.cube16() if which == "cube16" else random_grid((-20, -20, -20), 0.3)
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    # one step under the 6, 18 and 26 neighbourhoods is the ball of max_d2 1, 2 and 3
    for max_d2, c in ((1, 6), (2, 18), (3, 26)):
        margin = ctx.morph_voxels(d_pos, None, H.MORPH_MARGIN, c)[0]
        assert len(margin) > 0 and torch.equal(ctx.margin_ball(d_pos, None, max_d2)[0], margin), (which, c)
    for max_d2, c in ((3, 26), (1, 6)):           # the random grid has no voxel with all 26 neighbours, and a few with all 6
        eroded = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_ERODE, c)
        ball = ctx.erode_ball(d_pos, d_mrgb, max_d2)
        assert torch.equal(ball[0], eroded[0]) and torch.equal(ball[1], eroded[1]), (which, c)
    assert len(eroded[0]) > 0
    # closing and opening by a ball, against the model
    for max_d2 in (2, 5):
        for got, want in ((ctx.close_ball(d_pos, d_mrgb, max_d2), D.close_ball(pos, mrgb, max_d2)), (ctx.open_ball(d_pos, d_mrgb, max_d2), D.open_ball(pos, mrgb, max_d2))):
            assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1]), (which, max_d2)
    depth = ctx.depth_voxels(d_pos, d_mrgb, 1)
    assert len(depth[0]) == len(T.source_of(pos)) and int((depth[2].cpu().numpy() == D.FAR).sum()) == len(eroded[0])


@pytest.mark.parametrize("r", [5, 16])
def test_a_dilated_voxel_is_the_rasterised_ball(H, ctx, r):
    # ball_voxels holds the cells whose centres lie within r of the centre of the cell (3, -4, 5): d2 <= r^2 between cells
    one = cells((3, -4, 5))
    ball = ctx.ball_voxels((3.5, -3.5, 5.5), r)[0]
    grown = ctx.dilate_ball(on_device(one), None, r * r)[0]
    assert len(ball) == len(D.offsets(r * r)) and torch.equal(grown, ball)


def test_the_scorch_falloff_around_a_crater_in_the_sponge(H):
    with H.Context(32, 32) as c:
        c.set_menger(3, 0, MENGER_MRGB)
        before = c.get_voxels_device()
        assert len(before[0]) == 8000
        pos = before[0].cpu().numpy().astype(np.int64)
        lo = pos.min(axis=0)
        g = np.arange(-6, 7)                                                 # around lo + 20, in a solid corner: the sponge's own centre is a hole
        ball = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        ball = (ball[(ball ** 2).sum(axis=1) < 5.5 ** 2] + lo + 20).astype(np.int16)      # cells of the ball, voxels or not
        scene = {tuple(p): tuple(b) for p, b in zip(pos.tolist(), before[1].cpu().numpy().tolist())}
        assert any(tuple(p) in scene for p in ball.tolist())
        # 1. the crater
        d_ball = on_device(ball)
        c.clear_voxels_device(d_ball)
        # 2. the cells within 6 of it, each with its squared distance from the crater ...
        near, _, d2 = c.distance_voxels(d_ball, None, H.DISTANCE_FIELD, 36)
        # 3. ... which the soot fades with, on torch's side
        shade = (200 - 5 * d2.to(torch.int32)).to(torch.uint8)
        soot = torch.stack([torch.full_like(shade, 3), shade, shade, shade], dim=1).contiguous()
        hit = c.combine_voxels(near, soot, *c.get_voxels_device()[:1], None, H.LIST_INTERSECT)       # ... where the scene has voxels
        assert 0 < len(hit[0]) < len(near)
        # 4. written back
        c.edit_voxels_device(*hit)
        # 5. the same on a dict
        for p in ball.tolist():
            scene.pop(tuple(p), None)
        field = D.distance_np(ball, None, D.FIELD, 36)
        shades = set()
        for p, d in zip(field[0].tolist(), field[2].tolist()):
            if tuple(p) in scene:
                scene[tuple(p)] = (3, 200 - 5 * d, 200 - 5 * d, 200 - 5 * d)
                shades.add(d)
        got = c.get_voxels_device()
        order = sorted(scene, key=T.path_key)
        assert got[0].cpu().numpy().tolist() == [list(p) for p in order] and got[1].cpu().numpy().tolist() == [list(scene[p]) for p in order]
        assert len(shades) > 10 and max(shades) == 36
