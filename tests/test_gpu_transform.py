"""GPU: vxrt_transform_voxels_device (include/vxrt_transform.h) against its rule in Python (tests/transform_model.py).

Every case compares positions and bytes with the model for exact equality and checks guard bytes around out_pos and out_mrgb, that
pos and mrgb are unchanged, that a second call writes the same bytes, and that the count-only form agrees (check).  Small boxes are
walked by the model's loop over Python integers, large ones by its numpy walk, which tests/test_transform_cpu.py holds equal to
the loop."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import ray_families as R
import transform_model as T
from list_op_harness import Bytes, check_call, last_error, on_device

pytestmark = pytest.mark.gpu

MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)
LOOP_CELLS = 30000        # boxes up to this many cells are walked by the model's Python loop


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def affine(H, m, t, reserved=0):
    a = H.Affine()
    for i in range(3):
        for j in range(3):
            a.m[i][j] = int(m[i][j])
        a.t[i] = int(t[i])
    a.reserved = reserved
    return a


def raw(ctx, pos, mrgb, n, pull, box_min, box_max, out_pos, out_mrgb, cap, count=True):
    """The C call over raw addresses -> (status, *n_out)."""
    torch.cuda.synchronize()
    got = C.c_size_t(0xDEAD)
    lo = None if box_min is None else (C.c_int32 * 3)(*[int(v) for v in box_min])
    hi = None if box_max is None else (C.c_int32 * 3)(*[int(v) for v in box_max])
    rc = ctx._L.vxrt_transform_voxels_device(ctx._h, pos, mrgb, C.c_size_t(n), None if pull is None else C.byref(pull), lo, hi, out_pos, out_mrgb,
                                             C.c_size_t(cap), C.byref(got) if count else None)
    return rc, got.value


def model(pos, mrgb, m, t, box_min, box_max):
    cells = int(np.prod([max(0, int(b) - int(a)) for a, b in zip(box_min, box_max)]))
    return (T.transform if cells <= LOOP_CELLS else T.transform_np)(pos, mrgb, m, t, box_min, box_max)


def check(H, ctx, pos, mrgb, m, t, box_min, box_max, what, want=None, shift=0):
    """One list, map and box through every form of the call against the model -> (pos, mrgb) of the result."""
    pos = np.ascontiguousarray(pos, np.int16).reshape(-1, 3)
    mrgb = None if mrgb is None else np.ascontiguousarray(mrgb, np.uint8).reshape(-1, 4)
    want_pos, want_mrgb = model(pos, mrgb, m, t, box_min, box_max) if want is None else want
    pull = affine(H, m, t)
    return check_call(ctx, lambda ptr, *out: raw(ctx, *ptr, len(pos), pull, box_min, box_max, *out),
                      lambda dev, cap: ctx.transform_voxels(*dev, pull, box_min, box_max, cap=cap),
                      [("pos", pos), ("mrgb", mrgb)], want_pos, want_mrgb, what, shift)


def box_of(pos, grow=0):
    p = np.asarray(pos, np.int64)
    return tuple(int(v) - grow for v in p.min(0)), tuple(int(v) + 1 + grow for v in p.max(0))


def by_path(pos, mrgb):
    src = T.source_of(pos, mrgb)
    keys = sorted(src, key=T.path_key)
    return np.array(keys, np.int16).reshape(-1, 3), np.array([src[k] for k in keys], np.uint8).reshape(-1, 4)


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(32, 32) as c:      # no scene is loaded: the call needs none
        yield c


@pytest.fixture(scope="module")
def lists():
    return {"cube16": R.scene_voxels("cube16"), "shell": T.shell(), "random": T.random_cells()}


# ---- the smallest cases ------------------------------------------------------------------------------------------------------------
def test_one_voxel_the_empty_box_and_the_empty_list(H, ctx):
    m, t = T.identity()
    pos, mrgb = np.array([[3, -4, 5]], np.int16), np.array([[0x85, 1, 2, 3]], np.uint8)
    got = check(H, ctx, pos, mrgb, m, t, (3, -4, 5), (4, -3, 6), "one voxel, one cell")
    assert got[0].tolist() == [[3, -4, 5]] and got[1].tolist() == [[5, 1, 2, 3]]
    assert len(check(H, ctx, pos, mrgb, m, t, (4, -4, 5), (5, -3, 6), "the cell beside it")[0]) == 0
    for box in (((0, 0, 0), (0, 9, 9)), ((0, 5, 0), (9, 5, 9)), ((0, 0, 7), (9, 9, 3)), ((32768, 0, 0), (32768, 1, 1))):
        assert len(check(H, ctx, pos, mrgb, m, t, *box, f"the empty box {box}")[0]) == 0
    # an empty box and n == 0 touch no device pointer
    pull = affine(H, m, t)
    wild = C.c_void_p(8), C.c_void_p(3)
    assert raw(ctx, *wild, 5, pull, (0, 0, 0), (0, 9, 9), C.c_void_p(5), C.c_void_p(7), 4) == (0, 0)
    assert raw(ctx, *wild, 0, pull, (0, 0, 0), (9, 9, 9), C.c_void_p(5), C.c_void_p(7), 4) == (0, 0)
    assert raw(ctx, None, None, 0, pull, (0, 0, 0), (9, 9, 9), None, None, 0) == (0, 0)
    assert len(check(H, ctx, pos[:0], mrgb[:0], m, t, (0, 0, 0), (9, 9, 9), "n == 0")[0]) == 0


def test_one_position_in_four_colours(H, ctx):
    pos = np.array([[1, 2, 3]] * 4, np.int16)
    mrgb = np.array([[0x81, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [0xFF, 4, 5, 6]], np.uint8)
    got = check(H, ctx, pos, mrgb, *T.identity(), (0, 0, 0), (4, 4, 4), "four colours")
    assert got[0].tolist() == [[1, 2, 3]] and got[1].tolist() == [[0x7F, 4, 5, 6]]            # the last entry wins
    got = check(H, ctx, pos, mrgb, *T.scale(32768), (0, 0, 0), (8, 8, 8), "four colours at half scale")
    assert len(got[0]) == 8 and (got[1] == [0x7F, 4, 5, 6]).all()


# ---- cube16 and the shell under exact maps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube16", "shell"])
def test_identity_translations_and_scales(H, ctx, lists, name):
    pos, mrgb = lists[name]
    want = by_path(pos, mrgb)
    got = check(H, ctx, pos, mrgb, *T.identity(), *box_of(pos, 1), f"{name}: identity", want=want)
    assert len(got[0]) == len(pos)
    check(H, ctx, pos, None, *T.identity(), *box_of(pos, 1), f"{name}: identity, positions only", want=(want[0], None))
    for offset in ((1, 0, 0), (-9, 4, 17), (0, 0, -8), (-3, -3, -3)):        # across 0 on every axis
        moved = pos.astype(np.int64) + np.array(offset)
        check(H, ctx, pos, mrgb, *T.translation(offset), *box_of(moved, 2), f"{name} + {offset}", want=by_path(moved, mrgb))
    half = check(H, ctx, pos, mrgb, *T.scale(32768), (-20, -20, -20), (20, 20, 20), f"{name}: m = 1/2")
    assert len(half[0]) == 8 * len(pos)
    double = check(H, ctx, pos, mrgb, *T.scale(131072), (-20, -20, -20), (20, 20, 20), f"{name}: m = 2")
    assert len(double[0]) == sum(1 for p in pos.tolist() if all(v & 1 for v in p)) > 100


@pytest.mark.parametrize("name", ["cube16", "shell"])
def test_the_24_rotations_about_a_half_integer_pivot_and_back(H, ctx, lists, name):
    pos, mrgb = lists[name]
    want_pos, want_mrgb = by_path(pos, mrgb)
    twice_pivot = (5, -3, 7)
    big = (-18, -18, -18), (18, 18, 18)
    seen = set()
    for k, r in enumerate(T.axis_rotations()):
        there = check(H, ctx, pos, mrgb, *T.rotation_pull(r, twice_pivot), *big, f"{name}: rotation {k}")
        assert len(there[0]) == len(want_pos)
        seen.add(there[0].tobytes() + there[1].tobytes())
        inverse = [[r[j][i] for j in range(3)] for i in range(3)]
        check(H, ctx, there[0], there[1], *T.rotation_pull(inverse, twice_pivot), *big, f"{name}: rotation {k} and back", want=(want_pos, want_mrgb))
    assert len(seen) == 24


# ---- general rotations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cube16", "shell", "random"])
def test_general_rotations_into_their_box_and_into_a_box_that_cuts(H, ctx, lists, name):
    pos, mrgb = lists[name]
    lo, hi = pos.min(0).astype(int), pos.max(0).astype(int)
    centre = tuple(((lo + hi + 1) / 2).tolist())
    for k, r in enumerate(T.GENERAL_ROTATIONS):
        shift = (3 * k, -2, 1.5 * k)
        a = H.rigid_pull(r, centre, shift)
        m, t = [list(row) for row in a.m], list(a.t)
        box = H.rigid_box(lo, hi, r, centre, shift)
        whole = check(H, ctx, pos, mrgb, m, t, *box, f"{name}: rotation {k} into rigid_box")
        assert 0.9 * len(T.source_of(pos)) < len(whole[0]) < 1.1 * len(T.source_of(pos))
        mid = tuple((a + b) // 2 + 1 for a, b in zip(*box))
        cut = check(H, ctx, pos, mrgb, m, t, box[0], (mid[0], box[1][1], mid[2]), f"{name}: rotation {k} into a box that cuts")
        assert 0 < len(cut[0]) < len(whole[0])
        inside = {tuple(p) for p in cut[0].tolist()}
        assert inside == {tuple(p) for p in whole[0].tolist() if p[0] < mid[0] and p[2] < mid[2]}
        # the wrapper of the whole motion
        w_pos, w_mrgb = ctx.rotate_voxels(on_device(pos), on_device(mrgb), r, centre, shift)
        assert np.array_equal(w_pos.cpu().numpy(), whole[0]) and np.array_equal(w_mrgb.cpu().numpy(), whole[1])
    # a box far larger than the source: most blocks leave at the bounding-box test, and the result is the same
    wide = tuple(v - 60 for v in box[0]), tuple(v + 70 for v in box[1])
    far = check(H, ctx, pos, mrgb, m, t, *wide, f"{name}: a box far larger than the source", want=whole)
    assert np.array_equal(far[0], whole[0])


# ---- sizes on either side of a block, of the staged keys and of a wave ---------------------------------------------------------------
def test_boxes_of_2047_2048_and_2049_cells_and_odd_extents_across_zero(H, ctx, lists):
    pos, mrgb = lists["random"]
    for lo, ext in (((5, 3, 7), (23, 89, 1)), ((4, 4, 4), (8, 16, 16)), ((7, 9, 0), (3, 1, 683)), ((0, 2, 1), (2049, 1, 1)), ((1, 0, 3), (1, 2047, 1))):
        cells = ext[0] * ext[1] * ext[2]
        assert cells in (2047, 2048, 2049)
        hi = tuple(a + b for a, b in zip(lo, ext))
        got = check(H, ctx, pos, mrgb, *T.identity(), lo, hi, f"a box of {ext}")
        assert 0 < len(got[0]) < cells
    cube, colours = lists["cube16"]
    for lo, hi in (((-5, -7, -3), (6, 4, 10)), ((-1, -1, -1), (1, 1, 1)), ((-8, -3, -13), (9, 2, 0)), ((-11, 0, -2), (0, 13, 5))):
        got = check(H, ctx, cube, colours, *T.translation((1, -2, 3)), lo, hi, f"the box {lo} .. {hi}")
        assert len(got[0]) > 0


def test_sources_on_either_side_of_the_staged_keys_and_of_a_block(H, ctx, lists):
    pos, mrgb = by_path(*lists["random"])
    rng = np.random.default_rng(5)
    order = rng.permutation(len(pos))
    a = H.rigid_pull(T.GENERAL_ROTATIONS[1], (20, 20, 20), (1, 2, 3))
    turned = [list(row) for row in a.m], list(a.t)
    for unique in (1, 2, 1023, 1024, 1025, 2047, 2049, 4097):
        take = order[:unique]
        repeat = take[rng.integers(0, unique, unique // 7)]                   # some positions twice, in other colours
        p = np.concatenate([pos[take], pos[repeat]])
        c = np.concatenate([mrgb[take], rng.integers(0, 256, (len(repeat), 4)).astype(np.uint8)])
        assert len(T.source_of(p)) == unique
        got = check(H, ctx, p, c, *T.identity(), (0, 0, 0), (40, 40, 40), f"{unique} unique entries")
        assert len(got[0]) == unique
        got = check(H, ctx, p, c, *turned, (-12, -12, -12), (52, 52, 52), f"{unique} unique entries, turned")
        assert unique < 1023 or 0.8 * unique <= len(got[0]) <= 1.2 * unique       # as many cells as voxels, give or take the sampling


def test_results_of_255_256_and_257_voxels(H, ctx):
    line = np.zeros((300, 3), np.int16)
    line[:, 2] = np.arange(-150, 150)
    mrgb = np.stack([np.arange(300) & 0x7F, np.arange(300) & 0xFF, np.full(300, 9), np.full(300, 200)], -1).astype(np.uint8)
    for k in (1, 63, 64, 65, 255, 256, 257):
        got = check(H, ctx, line, mrgb, *T.identity(), (-1, -1, -150), (2, 2, -150 + k), f"{k} voxels")
        assert len(got[0]) == k


# ---- the ends of the int16 range ---------------------------------------------------------------------------------------------------
def test_the_corners_of_the_int16_range(H, ctx):
    corners = np.array([[x, y, z] for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)], np.int16)
    mrgb = np.stack([np.arange(8), np.arange(8) + 10, np.arange(8) + 20, np.arange(8) + 30], -1).astype(np.uint8)
    for k, c in enumerate(corners.tolist()):
        lo = tuple(v - 1 if v > 0 else v for v in c)
        hi = tuple(v + 2 for v in lo)
        got = check(H, ctx, corners, mrgb, *T.identity(), lo, hi, f"the corner {c}")
        assert got[0].tolist() == [c] and got[1].tolist() == [mrgb[k].tolist()]
    got = check(H, ctx, np.array([[32767, -32768, 0]], np.int16), mrgb[:1], *T.identity(), (32760, -32768, -4), (32768, -32760, 4), "(32767, -32768, 0)")
    assert got[0].tolist() == [[32767, -32768, 0]]


def test_a_pull_past_the_range_is_absent_not_wrapped(H, ctx):
    ys = np.arange(-20, 20)
    low = np.stack([np.full(40, -32768), ys, np.zeros(40, int)], -1)         # where a wrapped 32768 would land
    high = np.stack([np.full(40, 32767), ys, np.ones(40, int)], -1)
    pos = np.concatenate([low, high]).astype(np.int16)
    m, t = T.translation((-1, 0, 0))                                          # s = d + 1
    assert len(check(H, ctx, pos, None, m, t, (32767, -20, 0), (32768, 20, 2), "a row pulled to 32768")[0]) == 0
    got = check(H, ctx, pos, None, m, t, (32766, -20, 0), (32768, 20, 2), "... and the row beside it")
    assert len(got[0]) == 40 and (got[0][:, 0] == 32766).all() and (got[0][:, 2] == 1).all()
    m, t = T.translation((1, 0, 0))                                           # s = d - 1
    assert len(check(H, ctx, pos, None, m, t, (-32768, -20, 0), (-32767, 20, 2), "a row pulled to -32769")[0]) == 0
    got = check(H, ctx, pos, None, m, t, (-32768, -20, 0), (-32766, 20, 2), "... and the row beside it")
    assert len(got[0]) == 40 and (got[0][:, 0] == -32767).all() and (got[0][:, 2] == 0).all()
    # the largest map and offset the header allows: every centre is pulled far outside
    m, t = T.scale(T.M_LIMIT)[0], [T.T_LIMIT, -T.T_LIMIT, T.T_LIMIT]
    assert len(check(H, ctx, pos, None, m, t, (-20, -20, -20), (20, 20, 20), "the limits of the map")[0]) == 0


# ---- addresses, room ---------------------------------------------------------------------------------------------------------------
def test_lists_and_outputs_at_odd_addresses(H, ctx, lists):
    pos, mrgb = lists["shell"]
    a = H.rigid_pull(T.GENERAL_ROTATIONS[2], (0, 0, 0), (0.5, 0, 0))
    m, t = [list(row) for row in a.m], list(a.t)
    box = H.rigid_box(pos.min(0), pos.max(0), T.GENERAL_ROTATIONS[2], (0, 0, 0), (0.5, 0, 0))
    want = model(pos, mrgb, m, t, *box)
    for shift in (1, 2, 3, 7):
        check(H, ctx, pos, mrgb, m, t, *box, f"addresses = {shift} mod 16", want=want, shift=shift)
    check(H, ctx, pos, None, m, t, *box, "positions only at an odd address", want=(want[0], None), shift=5)


def test_room_for_exactly_the_count_and_for_one_less(H, ctx, lists):
    pos, mrgb = lists["cube16"]
    k = len(pos)
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    pull = affine(H, *T.identity())
    box = box_of(pos)
    args = (ctx, C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr()), k, pull, *box)
    out_pos, out_mrgb = Bytes(6 * k), Bytes(4 * k)
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, k - 1) == (H.E_INVALID, k)
    assert str(k) in last_error(ctx) and str(k - 1) in last_error(ctx) and "vxrt_transform_voxels_device" in last_error(ctx)
    assert out_pos.untouched() and out_mrgb.untouched()
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, 0) == (H.E_INVALID, k) and out_pos.untouched() and out_mrgb.untouched()
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, k) == (0, k) and out_pos.guards_hold() and out_mrgb.guards_hold()
    want = by_path(pos, mrgb)
    assert np.array_equal(out_pos.data().view(np.int16).reshape(-1, 3), want[0]) and np.array_equal(out_mrgb.data().reshape(-1, 4), want[1])
    with pytest.raises(H.VxrtError) as e:
        ctx.transform_voxels(d_pos, d_mrgb, pull, *box, cap=k - 1)
    assert e.value.status == H.E_INVALID


def test_refusals_write_nothing(H, ctx, lists):
    pos, mrgb = lists["cube16"]
    n = len(pos)
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    p, c = C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr())
    good = affine(H, *T.identity())
    lo, hi = box_of(pos)
    out_pos, out_mrgb = Bytes(6 * n), Bytes(4 * n)

    def refused(*args, status=H.E_INVALID, says=None, **kw):
        assert raw(ctx, *args, **kw) == (status, 0xDEAD), args
        assert last_error(ctx) and (says is None or says in last_error(ctx)), last_error(ctx)
        assert out_pos.untouched() and out_mrgb.untouched()

    refused(p, c, 1 << 32, good, lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="2^32")           # before any pointer is looked at
    refused(None, None, 1 << 32, None, None, None, None, None, 0, says="2^32")
    refused(p, c, n, None, lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="null")
    refused(p, c, n, good, None, hi, out_pos.ptr, out_mrgb.ptr, n, says="null")
    refused(p, c, n, good, lo, None, out_pos.ptr, out_mrgb.ptr, n, says="null")
    refused(p, c, n, good, lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="null", count=False)
    refused(p, c, n, affine(H, *T.identity(), reserved=1), lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="reserved")
    for i in range(3):
        for sign in (1, -1):
            m, t = T.identity()
            m[i][(i + 1) % 3] = sign * (T.M_LIMIT + 1)
            refused(p, c, n, affine(H, m, t), lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="2^24")
            m, t = T.identity()
            t[i] = sign * (T.T_LIMIT + 1)
            refused(p, c, n, affine(H, m, t), lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="2^40")
    for bad in ((-32769, 0, 0), (0, 32769, 0), (0, 0, -2 ** 31), (2 ** 31 - 1, 0, 0)):
        refused(p, c, n, good, bad, hi, out_pos.ptr, out_mrgb.ptr, n, says="corner")
        refused(p, c, n, good, lo, bad, out_pos.ptr, out_mrgb.ptr, n, says="corner")
    refused(p, c, n, good, (-32768, -32768, 0), (32768, 32768, 1), out_pos.ptr, out_mrgb.ptr, n, says="2^32 cells")
    refused(None, c, n, good, lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="null")
    refused(p, c, n, good, lo, hi, out_pos.ptr, None, n, says="both or neither")
    refused(p, c, n, good, lo, hi, None, out_mrgb.ptr, n, says="both or neither")
    refused(p, None, n, good, lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="without mrgb")
    refused(p, None, n, good, lo, hi, None, out_mrgb.ptr, n, says="without mrgb")
    # host memory, pageable and pinned
    refused(C.c_void_p(pos.ctypes.data), c, n, good, lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="pos")
    assert "not device memory" in last_error(ctx)
    pinned = torch.as_tensor(np.array(mrgb)).pin_memory()
    refused(p, C.c_void_p(pinned.data_ptr()), n, good, lo, hi, out_pos.ptr, out_mrgb.ptr, n, says="mrgb")
    host_pos, host_mrgb = np.zeros((n, 3), np.int16), np.zeros((n, 4), np.uint8)
    refused(p, c, n, good, lo, hi, C.c_void_p(host_pos.ctypes.data), out_mrgb.ptr, n, says="out_pos")
    refused(p, c, n, good, lo, hi, out_pos.ptr, C.c_void_p(host_mrgb.ctypes.data), n, says="out_mrgb")
    assert not host_pos.any() and not host_mrgb.any()
    # an output one entry short of its cap: an allocation of its own, because what the library can see is the allocation
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    room = 1025                                                                     # 1024 entries of 4 bytes are a whole page: no rounding hides the missing one
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (room - 1))) == 0
    refused(p, c, n, good, lo, hi, out_pos.ptr, short, room, says="past its allocation")
    assert "out_mrgb" in last_error(ctx)
    assert hip.hipFree(short) == 0
    # ... and the valid call is accepted afterwards
    assert raw(ctx, p, c, n, good, lo, hi, out_pos.ptr, out_mrgb.ptr, n) == (0, n) and out_pos.guards_hold() and out_mrgb.guards_hold()
    assert np.array_equal(d_pos.cpu().numpy(), pos) and np.array_equal(d_mrgb.cpu().numpy(), mrgb)


# ---- beside the calls it feeds -----------------------------------------------------------------------------------------------------
def test_identity_is_the_scene_set_voxels_device_builds(H, lists):
    pos, mrgb = lists["random"]
    with H.Context(32, 32) as c:
        d_pos, d_mrgb = on_device(pos), on_device(mrgb)
        c.set_voxels_device(d_pos, d_mrgb)
        s_pos, s_mrgb = c.get_voxels_device()
        t_pos, t_mrgb = c.transform_voxels(d_pos, d_mrgb, H.rigid_pull(np.eye(3)), (0, 0, 0), (40, 40, 40))
        assert len(s_pos) == len(T.source_of(pos)) < len(pos)
        assert torch.equal(s_pos, t_pos) and torch.equal(s_mrgb, t_mrgb)


def test_a_detached_piece_is_turned_tested_and_put_back(H):
    with H.Context(32, 32) as c:
        c.set_menger(3, 0, MENGER_MRGB)
        pos, mrgb = c.get_voxels()
        assert len(pos) == 8000
        lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
        anchor = (tuple(lo.tolist()), (int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))            # the lowest y layer
        cut = pos[:, 1] == lo[1] + 8
        c.clear_voxels_device(on_device(pos[cut]))
        p_pos, p_mrgb, piece, table = c.drop_detached_pieces(*anchor)
        assert table["voxels"].cpu().numpy().tolist() == [4800] and len(p_pos) == 4800
        piece_pos, piece_mrgb = p_pos.cpu().numpy(), p_mrgb.cpu().numpy()
        gone = {tuple(p) for p in piece_pos.tolist()}
        scene = {tuple(p): tuple(b) for p, b in zip(pos[~cut].tolist(), mrgb[~cut].tolist()) if tuple(p) not in gone}
        assert len(scene) == c.count_voxels()
        # about its centre of mass, lifted clear of what is left standing
        centre = tuple((table["sum"].cpu().numpy()[0] / 4800 + 0.5).tolist())
        r, shift = T.GENERAL_ROTATIONS[0], (1, 12, -2)
        t_pos, t_mrgb = c.rotate_voxels(p_pos, p_mrgb, r, centre, shift)
        a = H.rigid_pull(r, centre, shift)
        box = H.rigid_box(piece_pos.min(0), piece_pos.max(0), r, centre, shift)
        want_pos, want_mrgb = T.transform_np(piece_pos, piece_mrgb, [list(row) for row in a.m], list(a.t), *box)
        assert 4300 < len(want_pos) < 5300
        assert np.array_equal(t_pos.cpu().numpy(), want_pos) and np.array_equal(t_mrgb.cpu().numpy(), want_mrgb)
        # the collision test of the turned piece, then the edit
        hits = sum(1 for p in want_pos.tolist() if tuple(p) in scene)
        assert c.count_present(t_pos) == hits
        c.edit_voxels_device(t_pos, t_mrgb, grow=True)
        scene.update({tuple(p): tuple(b) for p, b in zip(want_pos.tolist(), want_mrgb.tolist())})
        g_pos, g_mrgb = c.get_voxels_device(*box)
        inside = sorted((k for k in scene if all(box[0][ax] <= k[ax] < box[1][ax] for ax in range(3))), key=T.path_key)
        assert len(g_pos) == len(inside) >= len(want_pos)
        assert np.array_equal(g_pos.cpu().numpy(), np.array(inside, np.int16)) and np.array_equal(g_mrgb.cpu().numpy(), np.array([scene[k] for k in inside], np.uint8))
        assert c.count_voxels() == len(scene)
