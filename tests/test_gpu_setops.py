"""GPU: vxrt_combine_voxels_device (include/vxrt_setops.h) against its rule in Python (tests/setops_model.py).

Every case compares positions and bytes with the model for exact equality and checks guard bytes around out_pos and out_mrgb, that
all four inputs are unchanged, that a second call writes the same bytes, that the count-only form agrees with and without a cap, and
the wrapper counting first and with room to spare (check: one helper, no lighter mode)."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import ray_families as R
import setops_model as S
import transform_model as T
from list_op_harness import Bytes, by_path, check_call, colours, last_error, on_device

pytestmark = pytest.mark.gpu

MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)
WITH_B_BYTES = (S.UNION, S.XOR, S.CHANGED)


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def raw(ctx, a_pos, a_mrgb, na, b_pos, b_mrgb, nb, op, out_pos, out_mrgb, cap, count=True):
    """The C call over raw addresses -> (status, *n_out)."""
    torch.cuda.synchronize()
    got = C.c_size_t(0xDEAD)
    rc = ctx._L.vxrt_combine_voxels_device(ctx._h, a_pos, a_mrgb, C.c_size_t(na), b_pos, b_mrgb, C.c_size_t(nb), C.c_uint32(op), out_pos, out_mrgb,
                                           C.c_size_t(cap), C.byref(got) if count else None)
    return rc, got.value


def check(ctx, a_pos, a_mrgb, b_pos, b_mrgb, op, what, shift=0, want=None):
    """Two lists and an op through every form of the call against the model -> (pos, mrgb) of the result.  want: the model's result,
    where the caller has it already."""
    what = f"{what}: {S.NAMES[op]}"
    a_pos, b_pos = (np.ascontiguousarray(p, np.int16).reshape(-1, 3) for p in (a_pos, b_pos))
    a_mrgb, b_mrgb = (None if c is None else np.ascontiguousarray(c, np.uint8).reshape(-1, 4) for c in (a_mrgb, b_mrgb))
    want_pos, want_mrgb = S.combine(a_pos, a_mrgb, b_pos, b_mrgb, op) if want is None else want
    return check_call(ctx, lambda ptr, *out: raw(ctx, ptr[0], ptr[1], len(a_pos), ptr[2], ptr[3], len(b_pos), op, *out),
                      lambda dev, cap: ctx.combine_voxels(*dev, op, cap=cap),
                      [("a_pos", a_pos), ("a_mrgb", a_mrgb), ("b_pos", b_pos), ("b_mrgb", b_mrgb)], want_pos, want_mrgb, what, shift)


def check_ops(ctx, a, b, what, shift=0):
    """All five ops with bytes -> the results' sizes."""
    return [len(check(ctx, *a, *b, op, what, shift)[0]) for op in S.OPS]


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(32, 32) as c:      # no scene is loaded: the call needs none
        yield c


@pytest.fixture(scope="module")
def pool():
    """6 000 distinct cells of [-20, 20)^3 in path order."""
    rng = np.random.default_rng(11)
    cells = np.argwhere(rng.random((40, 40, 40)) < 0.1)[:6000] - 20
    assert len(cells) == 6000
    return by_path(cells)


# ---- the smallest cases ------------------------------------------------------------------------------------------------------------
def test_one_voxel_against_itself_another_and_nothing(H, ctx):
    one, red = np.array([[3, -4, 5]], np.int16), np.array([[0x85, 1, 2, 3]], np.uint8)
    two, blue = np.array([[3, -4, 6]], np.int16), np.array([[7, 9, 9, 9]], np.uint8)
    none = (one[:0], red[:0])
    assert check_ops(ctx, (one, red), (one, red), "a voxel and itself") == [1, 1, 0, 0, 0]
    assert check_ops(ctx, (one, red), (one, blue), "a voxel and itself in another colour") == [1, 1, 0, 0, 1]
    assert check(ctx, one, red, one, blue, S.UNION, "last wins")[1].tolist() == [[7, 9, 9, 9]]
    assert check(ctx, one, red, one, blue, S.INTERSECT, "A's bytes")[1].tolist() == [[5, 1, 2, 3]]
    assert check_ops(ctx, (one, red), (two, blue), "a voxel and its neighbour") == [2, 0, 1, 2, 1]
    assert check_ops(ctx, (one, red), none, "a voxel and nothing") == [1, 0, 1, 1, 0]
    assert check_ops(ctx, none, (one, red), "nothing and a voxel") == [1, 0, 0, 1, 1]
    assert check_ops(ctx, none, none, "nothing and nothing") == [0, 0, 0, 0, 0]
    # bit 7 of the material byte never makes a voxel changed
    assert len(check(ctx, one, red, one, np.array([[0x05, 1, 2, 3]], np.uint8), S.CHANGED, "bit 7")[0]) == 0
    # two empty lists touch no device pointer; one empty list's pointers may be null
    wild = C.c_void_p(8), C.c_void_p(3)
    for op in S.OPS:
        assert raw(ctx, *wild, 0, *wild, 0, op, C.c_void_p(5), C.c_void_p(7), 4) == (0, 0)
    assert raw(ctx, None, None, 0, None, None, 0, S.XOR, None, None, 0) == (0, 0)
    d_pos, d_mrgb = on_device(one), on_device(red)
    p, c = C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr())
    assert raw(ctx, p, c, 1, None, None, 0, S.UNION, None, None, 0) == (0, 1), last_error(ctx)
    assert raw(ctx, None, c, 0, p, c, 1, S.CHANGED, None, None, 0) == (0, 1), last_error(ctx)
    assert raw(ctx, p, None, 1, None, None, 0, S.DIFFERENCE, None, None, 0) == (0, 1), last_error(ctx)


def test_one_position_in_four_colours_in_each_list(H, ctx):
    pos = np.array([[1, 2, 3]] * 4, np.int16)
    a = np.array([[0x81, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [0xFF, 4, 5, 6]], np.uint8)
    b = np.array([[0xFF, 4, 5, 6], [9, 9, 9, 9], [8, 8, 8, 8], [0x7F, 4, 5, 7]], np.uint8)
    assert check_ops(ctx, (pos, a), (pos, b), "four colours") == [1, 1, 0, 0, 1]
    assert check(ctx, pos, a, pos, b, S.UNION, "four colours")[1].tolist() == [[0x7F, 4, 5, 7]]          # the last entry of B
    assert check(ctx, pos, a, pos, b, S.INTERSECT, "four colours")[1].tolist() == [[0x7F, 4, 5, 6]]      # the last entry of A
    assert check_ops(ctx, (pos, a), (pos, b[[1, 2, 3, 0]]), "... and B ending as A does") == [1, 1, 0, 0, 0]


@pytest.mark.parametrize("pair", ["cube16 and cube16 + (8, 0, 0)", "the shell and the solid cube"])
def test_all_five_ops_on_overlapping_shapes(H, ctx, pair):
    cube = R.scene_voxels("cube16")
    if pair.startswith("cube16"):
        a, b = cube, ((cube[0].astype(np.int64) + (8, 0, 0)).astype(np.int16), colours(len(cube[0]), 2))
    else:
        g = np.arange(-9, 9)
        solid = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)      # the shell's cells and its inside
        a, b = T.shell(), (solid, colours(len(solid), 3))
    sizes = check_ops(ctx, a, b, pair)
    na, nb = len(by_path(a[0])), len(by_path(b[0]))
    assert sizes[S.UNION] == na + nb - sizes[S.INTERSECT] and sizes[S.DIFFERENCE] == na - sizes[S.INTERSECT] and 0 < sizes[S.INTERSECT] <= na
    assert sizes[S.XOR] == sizes[S.UNION] - sizes[S.INTERSECT] and sizes[S.CHANGED] == nb        # random bytes: every common voxel differs
    check_ops(ctx, b, a, pair + ", the other way round")
    for op in (S.UNION, S.INTERSECT, S.DIFFERENCE, S.XOR):
        check(ctx, a[0], None, b[0], None, op, pair + ", positions only")


# ---- pairs across every boundary ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra_in", ["A", "B"])
def test_pairs_that_straddle_every_thread_boundary_and_the_block_boundary(H, ctx, pool, extra_in):
    # B = 1 025 keys, A = B plus one voxel that sorts first: the equal pairs lie at merged items (2 k + 1, 2 k + 2), one across every
    # 8-item boundary and one across 2 047 / 2 048 (tests/test_setops_cpu.py: test_the_straddle_lists_straddle)
    more, fewer = pool[:1026], pool[1:1026]
    bytes_more = colours(1026, 4)
    bytes_fewer = bytes_more[1:].copy()
    a, b = ((more, bytes_more), (fewer, bytes_fewer)) if extra_in == "A" else ((fewer, bytes_fewer), (more, bytes_more))
    rng = np.random.default_rng(5)
    shuffled = lambda l: tuple(v[o] for o in [rng.permutation(len(l[0]))] for v in l)      # noqa: E731
    sizes = check_ops(ctx, shuffled(a), shuffled(b), f"the extra voxel in {extra_in}, equal words")
    assert sizes == [1026, 1025, 1 if extra_in == "A" else 0, 1, 0 if extra_in == "A" else 1]
    # one differing word exactly at the pair across merged items 2 047 / 2 048: pool[1024], the 1 024th key of the shorter list
    other = bytes_fewer.copy()
    other[1023, 2] ^= 1
    a, b = ((more, bytes_more), (fewer, other)) if extra_in == "A" else ((fewer, other), (more, bytes_more))
    got = check(ctx, *shuffled(a), *shuffled(b), S.CHANGED, f"the extra voxel in {extra_in}, one word differs at the block boundary")
    want = [pool[1024].tolist()] if extra_in == "A" else sorted([pool[0].tolist(), pool[1024].tolist()], key=T.path_key)
    assert got[0].tolist() == want


# ---- sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [2047, 2048, 2049, 4095, 4096, 4097])
def test_merged_lengths_on_either_side_of_a_block(H, ctx, pool, total):
    rng = np.random.default_rng(total)
    ma = total // 2 + 3
    a_pos, b_pos = pool[np.sort(rng.choice(total, ma, replace=False))], pool[np.sort(rng.choice(total, total - ma, replace=False))]
    sizes = check_ops(ctx, (a_pos, colours(ma, 6)), (b_pos, colours(total - ma, 7)), f"{total} merged items")
    assert 0 < sizes[S.INTERSECT] < ma and sizes[S.UNION] + sizes[S.INTERSECT] == total


def test_one_against_many_and_lists_that_do_not_interleave(H, ctx, pool):
    many, bytes_many = pool[:5000], colours(5000, 8)
    for k in (0, 2500, 4999):
        one = (pool[k:k + 1], colours(1, 9))
        assert check_ops(ctx, one, (many, bytes_many), f"ma = 1 (entry {k}), mb = 5 000")[:2] == [5000, 1]
        assert check_ops(ctx, (many, bytes_many), one, f"ma = 5 000, mb = 1 (entry {k})")[:2] == [5000, 1]
    assert check_ops(ctx, (pool[5500:5501], colours(1, 9)), (many, bytes_many), "ma = 1, past all of B")[:2] == [5001, 0]
    low, high = (pool[:2500], colours(2500, 10)), (pool[2500:4600], colours(2100, 12))
    assert check_ops(ctx, low, high, "all of A before all of B") == [4600, 0, 2500, 4600, 2100]
    assert check_ops(ctx, high, low, "all of B before all of A") == [4600, 0, 2100, 4600, 2500]
    same = (pool[:3000], colours(3000, 13))
    assert check_ops(ctx, same, same, "identical 3 000-entry lists") == [3000, 3000, 0, 0, 0]
    assert check_ops(ctx, same, (same[0], colours(3000, 14)), "... with other bytes")[S.CHANGED] == 3000


def test_results_of_0_and_255_to_257_voxels(H, ctx, pool):
    a = (pool[:600], colours(600, 15))
    for k in (0, 1, 63, 64, 65, 255, 256, 257):
        b_pos = np.concatenate([pool[300:300 + k], pool[1000:1400]])
        sizes = check_ops(ctx, a, (b_pos, colours(len(b_pos), 16)), f"{k} voxels in common")
        assert sizes[S.INTERSECT] == k and sizes[S.DIFFERENCE] == 600 - k
    b_pos = np.concatenate([pool[:600], pool[600:856]])
    assert check_ops(ctx, a, (b_pos, np.concatenate([a[1], colours(256, 17)])), "256 new voxels")[S.CHANGED] == 256


def test_lists_with_every_position_five_times(H, ctx, pool):
    rng = np.random.default_rng(18)
    a_cells, b_cells = pool[:4000], pool[2000:6000]
    lists = []
    for cells, seed in ((a_cells, 19), (b_cells, 20)):
        order = rng.permutation(5 * len(cells))
        lists.append((np.tile(cells, (5, 1))[order], colours(5 * len(cells), seed)[order]))
    assert check_ops(ctx, *lists, "every position five times, unsorted")[:4] == [6000, 2000, 2000, 4000]


def test_the_corners_of_the_int16_range(H, ctx):
    corners = np.array([[x, y, z] for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)], np.int16)
    mrgb = np.stack([np.arange(8), np.arange(8) + 10, np.arange(8) + 20, np.arange(8) + 30], -1).astype(np.uint8)
    inner = np.array([[0, 0, 0], [-1, -1, -1], [32767, 0, -32768]], np.int16)
    inner_bytes = colours(3, 21)
    a = (np.concatenate([corners[:6], inner]), np.concatenate([mrgb[:6], inner_bytes]))
    b = (np.concatenate([inner[:2], corners[2:]]), np.concatenate([inner_bytes[:2], mrgb[2:]]))
    assert check_ops(ctx, a, b, "the corners of the range") == [11, 6, 3, 5, 2]
    assert check(ctx, *a, *b, S.INTERSECT, "the corners")[0].tolist() == by_path(np.concatenate([corners[2:6], inner[:2]])).tolist()


# ---- addresses, values, room -------------------------------------------------------------------------------------------------------
def test_all_six_arrays_at_odd_addresses(H, ctx, pool):
    a, b = (pool[:1500], colours(1500, 23)), (pool[700:2300], colours(1600, 24))
    for shift in (1, 2, 3, 7):
        for op in S.OPS:
            check(ctx, *a, *b, op, f"addresses = {shift} mod 16", shift=shift)
    check(ctx, a[0], None, b[0], None, S.XOR, "positions only at an odd address", shift=5)


def test_positions_only_and_b_as_a_mask(H, ctx, pool):
    a, b = (pool[:1500], colours(1500, 25)), (pool[700:2300], colours(1600, 26))
    for op in (S.UNION, S.INTERSECT, S.DIFFERENCE, S.XOR):
        only = check(ctx, a[0], None, b[0], None, op, "positions only")
        full = check(ctx, *a, *b, op, "with bytes")
        assert only[1] is None and np.array_equal(only[0], full[0])
    for op in (S.INTERSECT, S.DIFFERENCE):
        masked, given = check(ctx, *a, b[0], None, op, "B as a mask"), check(ctx, *a, *b, op, "B with bytes that are ignored")
        assert np.array_equal(masked[0], given[0]) and np.array_equal(masked[1], given[1])


def test_room_for_exactly_the_count_and_for_one_less(H, ctx, pool):
    a, b = (pool[:1500], colours(1500, 27)), (pool[700:2300], colours(1600, 28))
    want = S.combine(*a, *b, S.UNION)
    k = len(want[0])
    dev = [on_device(v) for v in (*a, *b)]
    args = (ctx, C.c_void_p(dev[0].data_ptr()), C.c_void_p(dev[1].data_ptr()), 1500, C.c_void_p(dev[2].data_ptr()), C.c_void_p(dev[3].data_ptr()), 1600, S.UNION)
    out_pos, out_mrgb = Bytes(6 * k), Bytes(4 * k)
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, k - 1) == (H.E_INVALID, k)
    assert str(k) in last_error(ctx) and str(k - 1) in last_error(ctx) and "vxrt_combine_voxels_device" in last_error(ctx)
    assert out_pos.untouched() and out_mrgb.untouched()
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, 0) == (H.E_INVALID, k) and out_pos.untouched() and out_mrgb.untouched()
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, k) == (0, k) and out_pos.guards_hold() and out_mrgb.guards_hold()
    assert np.array_equal(out_pos.data().view(np.int16).reshape(-1, 3), want[0]) and np.array_equal(out_mrgb.data().reshape(-1, 4), want[1])
    with pytest.raises(H.VxrtError) as e:
        ctx.combine_voxels(*dev, H.LIST_UNION, cap=k - 1)
    assert e.value.status == H.E_INVALID


def test_refusals_write_nothing(H, ctx):
    pos, mrgb = R.scene_voxels("cube16")
    n = len(pos)
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    p, c = C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr())
    out_pos, out_mrgb = Bytes(6 * 2 * n), Bytes(4 * 2 * n)
    o, w, room = out_pos.ptr, out_mrgb.ptr, 2 * n

    def refused(*args, status=H.E_INVALID, says=None, **kw):
        assert raw(ctx, *args, **kw) == (status, 0xDEAD), args
        assert last_error(ctx) and (says is None or says in last_error(ctx)), last_error(ctx)
        assert out_pos.untouched() and out_mrgb.untouched()

    refused(p, c, 1 << 32, p, c, n, S.UNION, o, w, room, says="2^32")                    # before any pointer is looked at
    refused(p, c, n, p, c, 1 << 32, S.UNION, o, w, room, says="2^32")
    refused(None, None, 1 << 32, None, None, 1 << 32, 9, None, None, 0, says="2^32", count=False)
    refused(p, c, n, p, c, n, S.UNION, o, w, room, says="n_out", count=False)
    for op in (5, 6, 0xFFFFFFFF):
        refused(p, c, n, p, c, n, op, o, w, room, says="vxrt_list_op")
    for op in S.OPS:
        if op in WITH_B_BYTES:
            refused(p, c, n, p, None, n, op, o, w, room, says="b_mrgb")                  # these take bytes from B
        refused(p, c, n, p, c, n, op, o, None, room, says="both or neither")
        refused(p, c, n, p, c, n, op, None, w, room, says="both or neither")
        refused(p, None, n, p, c, n, op, o, None, room, says="b_mrgb without a_mrgb")
        refused(p, None, n, p, None, n, op, o, w, room, says="out_mrgb without a_mrgb")
    refused(p, None, n, p, None, n, S.CHANGED, None, None, 0, says="CHANGED")
    refused(None, c, n, p, c, n, S.UNION, o, w, room, says="null voxel positions")
    refused(p, c, n, None, c, n, S.UNION, o, w, room, says="null voxel positions")
    # host memory, pageable and pinned
    refused(C.c_void_p(pos.ctypes.data), c, n, p, c, n, S.UNION, o, w, room, says="a_pos")
    assert "not device memory" in last_error(ctx)
    pinned = torch.as_tensor(np.array(mrgb)).pin_memory()
    refused(p, C.c_void_p(pinned.data_ptr()), n, p, c, n, S.UNION, o, w, room, says="a_mrgb")
    refused(p, c, n, C.c_void_p(pos.ctypes.data), c, n, S.UNION, o, w, room, says="b_pos")
    refused(p, c, n, p, C.c_void_p(pinned.data_ptr()), n, S.UNION, o, w, room, says="b_mrgb")
    refused(p, c, n, p, C.c_void_p(pinned.data_ptr()), n, S.INTERSECT, o, w, room, says="b_mrgb")      # ignored, and checked all the same
    host_pos, host_mrgb = np.zeros((room, 3), np.int16), np.zeros((room, 4), np.uint8)
    refused(p, c, n, p, c, n, S.UNION, C.c_void_p(host_pos.ctypes.data), w, room, says="out_pos")
    refused(p, c, n, p, c, n, S.UNION, o, C.c_void_p(host_mrgb.ctypes.data), room, says="out_mrgb")
    assert not host_pos.any() and not host_mrgb.any()
    # an output one entry short of its cap: an allocation of its own, because what the library can see is the allocation
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    cap = 1025                                                                      # 1024 entries of 4 bytes are a whole page: no rounding hides the missing one
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (cap - 1))) == 0
    refused(p, c, n, p, c, n, S.UNION, o, short, cap, says="past its allocation")
    assert "out_mrgb" in last_error(ctx)
    assert hip.hipFree(short) == 0
    # ... and the valid call is accepted afterwards
    assert raw(ctx, p, c, n, p, c, n, S.UNION, o, w, room) == (0, n) and out_pos.guards_hold() and out_mrgb.guards_hold()
    assert np.array_equal(d_pos.cpu().numpy(), pos) and np.array_equal(d_mrgb.cpu().numpy(), mrgb)


def test_the_outputs_may_be_an_inputs_arrays(H, ctx, pool):
    rng = np.random.default_rng(30)
    order = rng.permutation(3000)
    a = (pool[:3000][order], colours(3000, 31))
    b = (pool[1000:4000], None)
    want = S.combine(*a, *b, S.DIFFERENCE)
    k = len(want[0])
    assert k == 1000
    io_pos, io_mrgb = Bytes(6 * 3000, 0, a[0]), Bytes(4 * 3000, 0, a[1])
    d_b = on_device(b[0])
    assert raw(ctx, io_pos.ptr, io_mrgb.ptr, 3000, C.c_void_p(d_b.data_ptr()), None, 3000, S.DIFFERENCE, io_pos.ptr, io_mrgb.ptr, 3000) == (0, k), last_error(ctx)
    assert io_pos.guards_hold() and io_mrgb.guards_hold()
    assert np.array_equal(io_pos.data()[:6 * k].view(np.int16).reshape(-1, 3), want[0]) and np.array_equal(io_mrgb.data()[:4 * k].reshape(-1, 4), want[1])
    # behind the result the input's bytes stand as they were
    assert io_pos.data()[6 * k:].tobytes() == a[0].tobytes()[6 * k:] and io_mrgb.data()[4 * k:].tobytes() == a[1].tobytes()[4 * k:]
    assert np.array_equal(d_b.cpu().numpy(), b[0])


# ---- beside the calls it stands for ------------------------------------------------------------------------------------------------
def test_union_and_difference_are_what_the_scene_route_gives(H, pool):
    rng = np.random.default_rng(32)
    a = (pool[:3000][rng.permutation(3000)], colours(3000, 33))
    b = (pool[2000:4500][rng.permutation(2500)], colours(2500, 34))
    dev = [on_device(v) for v in (*a, *b)]
    with H.Context(32, 32) as c:
        c.set_voxels_device(dev[0], dev[1])
        c.edit_voxels_device(dev[2], dev[3], grow=True)
        s_pos, s_mrgb = c.get_voxels_device()
        u_pos, u_mrgb = c.combine_voxels(*dev, H.LIST_UNION)
        assert len(u_pos) == 4500 and torch.equal(s_pos, u_pos) and torch.equal(s_mrgb, u_mrgb)
        c.set_voxels_device(dev[0], dev[1])
        c.clear_voxels_device(dev[2])
        s_pos, s_mrgb = c.get_voxels_device()
        d_pos, d_mrgb = c.combine_voxels(dev[0], dev[1], dev[2], None, H.LIST_DIFFERENCE)
        assert len(d_pos) == 2000 and torch.equal(s_pos, d_pos) and torch.equal(s_mrgb, d_mrgb)


def test_the_delta_of_an_edited_sponge_replays_and_undoes(H):
    with H.Context(32, 32) as c, H.Context(32, 32) as fresh:
        c.set_menger(3, 0, MENGER_MRGB)
        before = c.get_voxels_device()
        assert len(before[0]) == 8000
        pos = before[0].cpu().numpy().astype(np.int64)
        lo, hi = pos.min(axis=0), pos.max(axis=0)
        centre = lo + 20.0                                                   # in a solid corner: the sponge's own centre is a hole
        ball = pos[((pos + 0.5 - centre) ** 2).sum(axis=1) < 5.0 ** 2]
        slab = pos[(pos[:, 1] >= lo[1] + 3) & (pos[:, 1] < lo[1] + 6)]
        assert len(ball) > 0 and len(slab) > 0 and not {tuple(p) for p in ball.tolist()} & {tuple(p) for p in slab.tolist()}
        c.clear_voxels_device(on_device(ball.astype(np.int16)))
        c.edit_voxels_device(on_device(slab.astype(np.int16)), on_device(np.tile(np.array([[5, 200, 30, 40]], np.uint8), (len(slab), 1))))
        after = c.get_voxels_device()
        assert len(after[0]) != 8000
        # forward, on a fresh context holding `before`
        set_pos, set_mrgb, clear_pos = c.diff_voxels(*before, *after)
        assert len(clear_pos) == len(ball) and len(set_pos) == len(slab)
        fresh.set_voxels_device(*before)
        fresh.edit_voxels_device(set_pos, set_mrgb)
        fresh.clear_voxels_device(clear_pos)
        got = fresh.get_voxels_device()
        assert torch.equal(got[0], after[0]) and torch.equal(got[1], after[1])
        # backward, on the edited context: the undo
        set_pos, set_mrgb, clear_pos = c.diff_voxels(*after, *before)
        assert len(clear_pos) == 0 and len(set_pos) == len(ball) + len(slab)
        c.edit_voxels_device(set_pos, set_mrgb)
        c.clear_voxels_device(clear_pos)
        got = c.get_voxels_device()
        assert torch.equal(got[0], before[0]) and torch.equal(got[1], before[1])
        # two detached pieces of a carved sponge share no cell; a piece and itself share all of it
        cut = pos[(pos[:, 1] == lo[1] + 8) | (pos[:, 1] == lo[1] + 14)]
        c.clear_voxels_device(on_device(cut.astype(np.int16)))
        anchor = (tuple(int(v) for v in lo), (int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))          # the lowest y layer
        p_pos, p_mrgb, piece, table = c.drop_detached_pieces(*anchor)
        sizes = table["voxels"].cpu().numpy().tolist()
        assert len(sizes) >= 2
        which, cells = piece.cpu().numpy(), p_pos.cpu().numpy()
        first, second = np.ascontiguousarray(cells[which == 0]), np.ascontiguousarray(cells[which == 1])
        assert len(first) == sizes[0] and len(second) == sizes[1]
        assert c.count_common(first, second) == 0
        assert c.count_common(first, first) == sizes[0] and c.count_common(second, second) == sizes[1]
        assert c.count_common(p_pos, second) == sizes[1]
