"""GPU: vxrt_shape_voxels_device (include/vxrt_shape.h) against its rule in Python (tests/shape_model.py).

Every case goes through one ladder (check): the counting call, which ignores cap; two writing calls between guard bytes, at the
address shift given and compared byte for byte; the wrapper with cap=None and with room to spare.  Positions and bytes are compared
with the model for exact equality.  Small boxes are walked by the model's loop over Python integers, large ones by its numpy walk,
which tests/test_shape_cpu.py holds equal to the loop."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import shape_model as S
from list_op_harness import DEV, Bytes, by_path, last_error, on_device

pytestmark = pytest.mark.gpu

MRGB = (0x85, 0xB0, 0xD0, 0x60)
LOOP_CELLS = 30000        # boxes up to this many cells are walked by the model's Python loop


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def shape_of(H, kind, r, h, reserved=(0, 0, 0)):
    s = H.Shape()
    s.kind, s.r = int(kind), int(r)
    for i in range(3):
        s.h[i], s.reserved[i] = int(h[i]), int(reserved[i])
    return s


def affine(H, m, t, reserved=0):
    a = H.Affine()
    for i in range(3):
        for j in range(3):
            a.m[i][j] = int(m[i][j])
        a.t[i] = int(t[i])
    a.reserved = reserved
    return a


def raw(ctx, shape, pull, box_min, box_max, mrgb, out_pos, out_mrgb, cap, count=True):
    """The C call -> (status, *n_out)."""
    torch.cuda.synchronize()
    got = C.c_size_t(0xDEAD)
    lo = None if box_min is None else (C.c_int32 * 3)(*[int(v) for v in box_min])
    hi = None if box_max is None else (C.c_int32 * 3)(*[int(v) for v in box_max])
    word = None if mrgb is None else (C.c_uint8 * 4)(*mrgb)
    rc = ctx._L.vxrt_shape_voxels_device(ctx._h, None if shape is None else C.byref(shape), None if pull is None else C.byref(pull), lo, hi, word,
                                         out_pos, out_mrgb, C.c_size_t(cap), C.byref(got) if count else None)
    return rc, got.value


def model(kind, r, h, m, t, box_min, box_max, mrgb):
    cells = int(np.prod([max(0, int(b) - int(a)) for a, b in zip(box_min, box_max)]))
    return (S.shape if cells <= LOOP_CELLS else S.shape_np)(kind, r, h, m, t, box_min, box_max, mrgb)


def check(H, ctx, kind, r, h, m, t, box_min, box_max, mrgb, what, want=None, shift=0, odd=3):
    """One shape, map and box through every form of the call against the model -> (pos, mrgb) of the result."""
    want_pos, want_mrgb = model(kind, r, h, m, t, box_min, box_max, mrgb) if want is None else want
    k = len(want_pos)
    shape, pull = shape_of(H, kind, r, h), affine(H, m, t)
    args = (ctx, shape, pull, box_min, box_max, mrgb)
    assert raw(*args, None, None, 0) == (0, k), (what, "count only", last_error(ctx))
    assert raw(*args, None, None, 12345) == (0, k), (what, "count only ignores cap")
    outs = []
    for turn, at in enumerate((shift, odd)):
        out_pos, out_mrgb = Bytes(6 * k, at), (Bytes(4 * k, at) if mrgb is not None else None)
        assert raw(*args, out_pos.ptr, None if out_mrgb is None else out_mrgb.ptr, k) == (0, k), (what, f"call {turn}", last_error(ctx))
        assert out_pos.guards_hold() and (out_mrgb is None or out_mrgb.guards_hold()), f"{what}: guard bytes"
        outs.append((out_pos, out_mrgb))
    got_pos = outs[0][0].data().view(np.int16).reshape(-1, 3)
    assert np.array_equal(got_pos, want_pos), f"{what}: {int((got_pos != want_pos).any(axis=1).sum())} of {k} positions differ"
    assert outs[1][0].data().tobytes() == outs[0][0].data().tobytes(), f"{what}: a second call, at an odd address"
    got_mrgb = None
    if mrgb is not None:
        got_mrgb = outs[0][1].data().reshape(-1, 4)
        assert np.array_equal(got_mrgb, want_mrgb), f"{what}: {int((got_mrgb != want_mrgb).any(axis=1).sum())} of {k} voxels' bytes differ"
        assert outs[1][1].data().tobytes() == outs[0][1].data().tobytes(), f"{what}: a second call, at an odd address"
    for cap in (None, k + 3):
        w_pos, w_mrgb = ctx.shape_voxels(shape, pull, box_min, box_max, mrgb, cap)
        assert w_pos.dtype == torch.int16 and w_pos.device == DEV and tuple(w_pos.shape) == (k, 3), what
        assert np.array_equal(w_pos.cpu().numpy(), want_pos), f"{what}: the wrapper"
        assert (w_mrgb is None) == (mrgb is None)
        if mrgb is not None:
            assert w_mrgb.dtype == torch.uint8 and tuple(w_mrgb.shape) == (k, 4) and np.array_equal(w_mrgb.cpu().numpy(), want_mrgb), f"{what}: the wrapper"
    return got_pos, got_mrgb


def check_made(H, ctx, made, mrgb, what, box=None, **kw):
    kind, r, h, m, t, lo, hi = S.unpack(H, made)
    lo, hi = (lo, hi) if box is None else box
    return check(H, ctx, kind, r, h, m, t, lo, hi, mrgb, what, **kw)


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(32, 32) as c:      # no scene is loaded: the call needs none
        yield c


@pytest.fixture(scope="module")
def ball30():
    """The ball of radius 30 about the corner (0, 0, 0) in [-40, 40)^3, computed once."""
    return S.shape_np(S.BALL, 30 * S.ONE, (0, 0, 0), *S.centred((0, 0, 0)), (-40, -40, -40), (40, 40, 40), MRGB)


KINDS = {"box": (S.BOX, 0, (9 * S.ONE, 13 * S.ONE, S.q16(6.5))), "ball": (S.BALL, S.q16(14.25), (0, 0, 0)),
         "cylinder": (S.CYLINDER, S.q16(9.5), (0, 0, 12 * S.ONE)), "capsule": (S.CAPSULE, S.q16(7.75), (0, 0, 9 * S.ONE))}


# ---- the four kinds under the identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(KINDS))
def test_each_kind_under_the_identity_in_a_box_off_the_tiles(H, ctx, name):
    kind, r, h = KINDS[name]
    lo = (-21, 3, 9)
    hi = tuple(v + 40 for v in lo)
    m, t = S.centred((-1, 23, 29))
    got = check(H, ctx, kind, r, h, m, t, lo, hi, MRGB, f"{name} with bytes")
    assert len(got[0]) > 1000 and (got[1] == [5, 0xB0, 0xD0, 0x60]).all()
    only = check(H, ctx, kind, r, h, m, t, lo, hi, None, f"{name}, positions only", shift=6, odd=1)
    assert np.array_equal(only[0], got[0]) and only[1] is None
    assert np.array_equal(got[0], by_path(got[0]))                     # in path order, each cell once


# ---- the shortcuts -----------------------------------------------------------------------------------------------------------------
def test_tiles_wholly_inside_wholly_outside_and_mixed(H, ctx, ball30):
    m, t = S.centred((0, 0, 0))
    got = check(H, ctx, S.BALL, 30 * S.ONE, (0, 0, 0), m, t, (-40, -40, -40), (40, 40, 40), MRGB, "the ball of radius 30", want=ball30)
    assert len(got[0]) == 113104
    cells = {tuple(p) for p in got[0].tolist()}
    tiles = [(x, y, z) for x in range(-48, 48, 16) for y in range(-48, 48, 16) for z in range(-48, 48, 16)]
    inside = [o for o in tiles if all((o[0] + i, o[1] + j, o[2] + k) in cells for i in (0, 15) for j in (0, 15) for k in (0, 15))]
    outside = [o for o in tiles if not any((o[0] + i, o[1] + j, o[2] + k) in cells for i in range(16) for j in range(16) for k in range(16))]
    assert len(inside) == 8 and len(outside) >= 8 and len(tiles) - len(inside) - len(outside) > 50


def test_a_box_that_cuts_the_ball_and_its_tiles(H, ctx, ball30):
    m, t = S.centred((0, 0, 0))
    lo, hi = (-13, -40, -7), (11, 5, 40)               # cuts the tiles wholly inside on every axis
    keep = ((ball30[0] >= lo) & (ball30[0] < hi)).all(axis=1)
    got = check(H, ctx, S.BALL, 30 * S.ONE, (0, 0, 0), m, t, lo, hi, MRGB, "the ball cut by a box", want=(ball30[0][keep], ball30[1][keep]))
    assert 0 < len(got[0]) < 113104
    one = check(H, ctx, S.BALL, 30 * S.ONE, (0, 0, 0), m, t, (-5, -5, -5), (6, 6, 6), None, "a box inside one tile's reach of the centre")
    assert len(one[0]) == 11 ** 3                                       # every tile it meets is wholly inside


# ---- the ends of the range ---------------------------------------------------------------------------------------------------------
def test_boxes_that_touch_the_ends_of_the_range(H, ctx):
    for ax in range(3):
        for end in (-32768, 32768):
            c = [5, -7, 11]
            c[ax] = end
            lo = [v - 9 for v in c]
            hi = [v + 9 for v in c]
            lo[ax], hi[ax] = max(lo[ax], -32768), min(hi[ax], 32768)
            got = check(H, ctx, S.BALL, S.q16(7.5), (0, 0, 0), *S.centred(c), lo, hi, MRGB, f"a ball about {c}")
            assert len(got[0]) > 500 and (got[0][:, ax] == (end if end < 0 else end - 1)).any()
    got = check(H, ctx, S.BOX, 0, (3 * S.ONE,) * 3, *S.centred((32768, -32768, 32768)), (32700, -32768, 32700), (32768, -32700, 32768), None, "a box at a corner")
    assert len(got[0]) == 27 and got[0].max() == 32767 and got[0].min() == -32768


# ---- thin boxes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 2])
def test_a_thin_box_through_a_capsule_along_it(H, ctx, axis):
    a, b = [3.5, -2.5, 7.5], [3.5, -2.5, 7.5]
    a[axis], b[axis] = -2000.0, 1900.5
    made = H.capsule_shape(a, b, 3.25)
    lo, hi = [3, -3, 7], [4, -2, 8]
    lo[axis], hi[axis] = -2500, 2500
    got = check_made(H, ctx, made, MRGB, f"a 5000-cell line along axis {axis}", box=(lo, hi))
    assert 3900 < len(got[0]) < 3915 and got[0][:, axis].min() < -2000 and got[0][:, axis].max() > 1901


# ---- maps --------------------------------------------------------------------------------------------------------------------------
def about(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(np.deg2rad(degrees)) * k + (1 - np.cos(np.deg2rad(degrees))) * (k @ k)


def test_a_rigid_pull_a_mirror_and_a_scaling_pull(H, ctx):
    rot = about((1, 2, 3), 37.0)
    turned = check_made(H, ctx, H.box_shape((4.5, -11, 20.25), (12, 5, 8.5), rot), MRGB, "a box turned 37 degrees about (1, 2, 3)")
    assert 0.9 * 8 * 12 * 5 * 8.5 < len(turned[0]) < 1.1 * 8 * 12 * 5 * 8.5
    check_made(H, ctx, H.cylinder_shape((-10, 4, 2), (13, -9, 21), 4.5), None, "a slanted cylinder")
    check_made(H, ctx, H.capsule_shape((-10, 4, 2), (13, -9, 21), 4.5), MRGB, "a slanted capsule")
    # a mirror: x -> -x about the plane x = 3 composed with the turn (determinant -1)
    kind, r, h, m, t, lo, hi = S.unpack(H, H.box_shape((4.5, -11, 20.25), (12, 5, 8.5), rot))
    mm = [[-row[0], row[1], row[2]] for row in m]
    tt = [t[i] + 2 * 3 * m[i][0] for i in range(3)]                       # M' x + t' = M (6 - x, y, z) + t
    lo2, hi2 = (6 - hi[0], lo[1], lo[2]), (6 - lo[0], hi[1], hi[2])
    mirrored = check(H, ctx, kind, r, h, mm, tt, lo2, hi2, MRGB, "the turned box mirrored")
    assert sorted((5 - p[0], p[1], p[2]) for p in mirrored[0].tolist()) == sorted(tuple(p) for p in turned[0].tolist())
    # a scaling pull
    egg = check_made(H, ctx, H.ellipsoid_shape((2.5, 3, -4), (5, 9, 14), rot), MRGB, "an ellipsoid with radii 5, 9 and 14")
    volume = 4 / 3 * np.pi * 5 * 9 * 14
    assert 0.95 * volume < len(egg[0]) < 1.05 * volume


def test_the_zero_matrix(H, ctx):
    zero = [[0] * 3] * 3
    lo, hi = (-9, 2, -30), (12, 20, 5)
    for kind, r, h in KINDS.values():
        got = check(H, ctx, kind, r, h, zero, [S.ONE, -2 * S.ONE, 3 * S.ONE], lo, hi, MRGB, f"kind {kind}: every centre pulled inside")
        assert len(got[0]) == 21 * 18 * 35
        got = check(H, ctx, kind, r, h, zero, [40 * S.ONE, 0, 0], lo, hi, MRGB, f"kind {kind}: every centre pulled outside")
        assert len(got[0]) == 0


# ---- rule 2 and the limits ---------------------------------------------------------------------------------------------------------
def test_a_centre_pulled_past_2_31_is_outside_not_wrapped(H, ctx):
    zero = [[0] * 3] * 3
    lo, hi = (-20, -20, -20), (20, 20, 20)
    # (2^41)^2 = 0 mod 2^64: squared without rule 2 the whole box would be inside
    for t in ([1 << 40, 0, 0], [0, -(1 << 40), 0], [0, 0, 1 << 40], [1 << 39, 1 << 39, 1 << 39]):
        for kind, r, h in ((S.BALL, S.ONE, (0, 0, 0)), (S.CAPSULE, S.ONE, (0, 0, S.ONE)), (S.CYLINDER, S.ONE, (0, 0, S.ONE))):
            assert len(check(H, ctx, kind, r, h, zero, t, lo, hi, MRGB, f"kind {kind}, t = {t}")[0]) == 0
    # |P| = 2^31 exactly is outside, one step nearer is inside the largest capsule's reach
    big = S.LIMIT
    assert len(check(H, ctx, S.CAPSULE, big, (0, 0, big), zero, [0, 0, 1 << 30], lo, hi, None, "P_2 = 2^31")[0]) == 0
    assert len(check(H, ctx, S.CAPSULE, big, (0, 0, big), zero, [0, 0, -(1 << 30)], lo, hi, None, "P_2 = -2^31")[0]) == 0
    assert len(check(H, ctx, S.CAPSULE, big, (0, 0, big), zero, [0, 0, (1 << 30) - 1], lo, hi, None, "P_2 = 2^31 - 2")[0]) == 40 ** 3


def test_the_limits_of_the_map_and_of_the_shape(H, ctx):
    big_m, big = S.M_LIMIT, S.LIMIT
    m = [[big_m, 0, 0], [0, big_m, 0], [0, 0, big_m]]                     # 256 shape cells per cell: radius 8192 is 32 cells
    lo, hi = (-40, -40, -40), (40, 40, 40)
    got = check(H, ctx, S.BALL, big, (0, 0, 0), m, [0, 0, 0], lo, hi, MRGB, "m = 2^24, r = 2^29")
    assert np.array_equal(got[0], S.shape_np(S.BALL, 32 * S.ONE, (0, 0, 0), *S.centred((0, 0, 0)), lo, hi)[0])
    check(H, ctx, S.BOX, 0, (big, big, big), m, [-S.T_LIMIT // (1 << 12), 0, 0], lo, hi, None, "the largest box")
    check(H, ctx, S.CAPSULE, big, (0, 0, big), [[-big_m, big_m, 0], [big_m, big_m, big_m], [0, -big_m, big_m]], [0, 0, 0], lo, hi, MRGB, "the largest capsule")
    assert len(check(H, ctx, S.BALL, big, (0, 0, 0), m, [S.T_LIMIT, -S.T_LIMIT, S.T_LIMIT], lo, hi, None, "t = 2^40")[0]) == 0


def test_degenerate_shapes(H, ctx):
    lo, hi = (-5, -5, -5), (6, 6, 6)
    assert len(check(H, ctx, S.BALL, 0, (0, 0, 0), *S.centred((0, 0, 0)), lo, hi, MRGB, "r = 0 about a corner")[0]) == 0
    got = check(H, ctx, S.BALL, 0, (0, 0, 0), S.identity()[0], [-S.ONE // 2] * 3, lo, hi, MRGB, "r = 0 about a centre")
    assert got[0].tolist() == [[0, 0, 0]]
    assert len(check(H, ctx, S.BOX, 0, (0, S.ONE, S.ONE), *S.centred((0, 0, 0)), lo, hi, MRGB, "a box with h = 0")[0]) == 0
    assert len(check(H, ctx, S.CYLINDER, 3 * S.ONE, (0, 0, 0), *S.centred((0, 0, 0)), lo, hi, MRGB, "a cylinder with h = 0")[0]) == 0
    both = check(H, ctx, S.CAPSULE, 3 * S.ONE, (0, 0, 0), *S.centred((0, 0, 0)), lo, hi, MRGB, "a capsule with h = 0")
    assert len(both[0]) == 136
    for box in (((0, 0, 0), (0, 9, 9)), ((0, 5, 0), (9, 5, 9)), ((0, 0, 7), (9, 9, 3)), ((32768, 0, 0), (32768, 1, 1))):
        assert len(check(H, ctx, S.BALL, 3 * S.ONE, (0, 0, 0), *S.centred((0, 0, 0)), *box, MRGB, f"the empty box {box}")[0]) == 0
    # an empty box touches no device pointer
    shape, pull = shape_of(H, S.BALL, S.ONE, (0, 0, 0)), affine(H, *S.identity())
    assert raw(ctx, shape, pull, (0, 0, 0), (0, 9, 9), MRGB, C.c_void_p(5), C.c_void_p(7), 4) == (0, 0)


# ---- room and refusals -------------------------------------------------------------------------------------------------------------
def test_room_for_exactly_the_count_and_for_one_less(H, ctx):
    shape, pull = shape_of(H, S.BALL, 3 * S.ONE, (0, 0, 0)), affine(H, *S.centred((0, 0, 0)))
    args = (ctx, shape, pull, (-5, -5, -5), (5, 5, 5), MRGB)
    k = 136
    out_pos, out_mrgb = Bytes(6 * k), Bytes(4 * k)
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, k - 1) == (H.E_INVALID, k)
    assert str(k) in last_error(ctx) and str(k - 1) in last_error(ctx) and "vxrt_shape_voxels_device" in last_error(ctx)
    assert out_pos.untouched() and out_mrgb.untouched()
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, 0) == (H.E_INVALID, k) and out_pos.untouched() and out_mrgb.untouched()
    assert raw(*args, out_pos.ptr, out_mrgb.ptr, k) == (0, k) and out_pos.guards_hold() and out_mrgb.guards_hold()
    want = S.shape(S.BALL, 3 * S.ONE, (0, 0, 0), *S.centred((0, 0, 0)), (-5, -5, -5), (5, 5, 5), MRGB)
    assert np.array_equal(out_pos.data().view(np.int16).reshape(-1, 3), want[0]) and np.array_equal(out_mrgb.data().reshape(-1, 4), want[1])
    with pytest.raises(H.VxrtError) as e:
        ctx.shape_voxels(shape, pull, (-5, -5, -5), (5, 5, 5), MRGB, cap=k - 1)
    assert e.value.status == H.E_INVALID


def test_refusals_write_nothing(H, ctx):
    n = 136
    good_shape, good = shape_of(H, S.BALL, 3 * S.ONE, (0, 0, 0)), affine(H, *S.centred((0, 0, 0)))
    lo, hi = (-5, -5, -5), (5, 5, 5)
    out_pos, out_mrgb = Bytes(6 * n), Bytes(4 * n)

    def refused(*args, status=H.E_INVALID, says=None, **kw):
        assert raw(ctx, *args, **kw) == (status, 0xDEAD), args
        assert last_error(ctx) and (says is None or says in last_error(ctx)), last_error(ctx)
        assert out_pos.untouched() and out_mrgb.untouched()

    # in the documented order: each call has everything later in the order wrong as well, where it can
    bad_pull, bad_shape, bad_box = affine(H, *S.identity(), reserved=1), shape_of(H, 4, 0, (0, 0, 0)), (-32769, 0, 0)
    refused(None, bad_pull, bad_box, hi, MRGB, out_pos.ptr, None, n, says="null")
    refused(good_shape, None, bad_box, hi, MRGB, out_pos.ptr, None, n, says="null")
    refused(good_shape, good, None, hi, MRGB, out_pos.ptr, out_mrgb.ptr, n, says="null")
    refused(good_shape, good, lo, None, MRGB, out_pos.ptr, out_mrgb.ptr, n, says="null")
    refused(good_shape, good, lo, hi, MRGB, out_pos.ptr, out_mrgb.ptr, n, says="null", count=False)
    refused(bad_shape, bad_pull, bad_box, hi, MRGB, out_pos.ptr, None, n, says="pull->reserved")
    for i in range(3):
        for sign in (1, -1):
            m, t = S.identity()
            m[i][(i + 1) % 3] = sign * (S.M_LIMIT + 1)
            refused(bad_shape, affine(H, m, t), bad_box, hi, MRGB, out_pos.ptr, None, n, says="2^24")
            m, t = S.identity()
            t[i] = sign * (S.T_LIMIT + 1)
            refused(bad_shape, affine(H, m, t), bad_box, hi, MRGB, out_pos.ptr, None, n, says="2^40")
    refused(bad_shape, good, bad_box, hi, MRGB, out_pos.ptr, None, n, says="kind")
    refused(shape_of(H, 0xFFFFFFFF, 0, (0, 0, 0)), good, lo, hi, MRGB, out_pos.ptr, out_mrgb.ptr, n, says="kind")
    refused(shape_of(H, S.BALL, S.LIMIT + 1, (0, 0, 0)), good, bad_box, hi, MRGB, out_pos.ptr, None, n, says="2^29")
    for i in range(3):
        h = [0, 0, 0]
        h[i] = S.LIMIT + 1
        refused(shape_of(H, S.BOX, 0, h), good, bad_box, hi, MRGB, out_pos.ptr, None, n, says="2^29")
    for kind, r, h in ((S.BOX, 1, (5, 5, 5)), (S.BALL, 5, (1, 0, 0)), (S.BALL, 5, (0, 1, 0)), (S.BALL, 5, (0, 0, 1)), (S.CYLINDER, 5, (1, 0, 5)),
                       (S.CYLINDER, 5, (0, 1, 5)), (S.CAPSULE, 5, (1, 0, 5)), (S.CAPSULE, 5, (0, 1, 5))):
        refused(shape_of(H, kind, r, h), good, bad_box, hi, MRGB, out_pos.ptr, None, n, says="does not use")
    for i in range(3):
        reserved = [0, 0, 0]
        reserved[i] = 1
        refused(shape_of(H, S.BALL, 5, (0, 0, 0), reserved), good, bad_box, hi, MRGB, out_pos.ptr, None, n, says="shape->reserved")
    for bad in ((-32769, 0, 0), (0, 32769, 0), (0, 0, -2 ** 31), (2 ** 31 - 1, 0, 0)):
        refused(good_shape, good, bad, hi, MRGB, out_pos.ptr, None, n, says="corner")
        refused(good_shape, good, lo, bad, MRGB, out_pos.ptr, None, n, says="corner")
    refused(good_shape, good, (-32768, -32768, 0), (32768, 32768, 1), MRGB, out_pos.ptr, None, n, says="2^32 cells")
    refused(good_shape, good, lo, hi, MRGB, out_pos.ptr, None, n, says="both or neither")
    refused(good_shape, good, lo, hi, MRGB, None, out_mrgb.ptr, n, says="both or neither")
    refused(good_shape, good, lo, hi, None, out_pos.ptr, out_mrgb.ptr, n, says="without mrgb")
    refused(good_shape, good, lo, hi, None, None, out_mrgb.ptr, n, says="without mrgb")
    # host memory, pageable and pinned
    host_pos, host_mrgb = np.zeros((n, 3), np.int16), np.zeros((n, 4), np.uint8)
    refused(good_shape, good, lo, hi, MRGB, C.c_void_p(host_pos.ctypes.data), out_mrgb.ptr, n, says="out_pos")
    assert "not device memory" in last_error(ctx)
    pinned = torch.zeros((n, 4), dtype=torch.uint8).pin_memory()
    refused(good_shape, good, lo, hi, MRGB, out_pos.ptr, C.c_void_p(pinned.data_ptr()), n, says="out_mrgb")
    assert not host_pos.any() and not host_mrgb.any() and not pinned.any()
    # an output one entry short of its cap: an allocation of its own, because what the library can see is the allocation
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    room = 1025                                                                     # 1024 entries of 4 bytes are a whole page: no rounding hides the missing one
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (room - 1))) == 0
    big_pos = Bytes(6 * room)
    refused(good_shape, good, lo, hi, MRGB, big_pos.ptr, short, room, says="past its allocation")
    assert "out_mrgb" in last_error(ctx) and big_pos.untouched()
    assert hip.hipFree(short) == 0
    # ... and the valid call is accepted afterwards
    assert raw(ctx, good_shape, good, lo, hi, MRGB, out_pos.ptr, out_mrgb.ptr, n) == (0, n) and out_pos.guards_hold() and out_mrgb.guards_hold()


# ---- beside the calls it feeds -----------------------------------------------------------------------------------------------------
def test_a_crater_a_beam_and_a_scene_of_its_own(H):
    with H.Context(64, 64) as c:
        c.set_menger(2, 0, (0, 0xB0, 0xD0, 0x60))
        pos, mrgb = c.get_voxels()
        scene = {tuple(p): tuple(b) for p, b in zip(pos.tolist(), mrgb.tolist())}
        assert len(scene) == 400
        lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int) + 1
        # a crater: the ball about one corner of the sponge
        corner = tuple(int(v) for v in hi)
        b_pos, none = c.ball_voxels(corner, 4.5)
        want = S.shape(*S.unpack(H, H.ball_shape(corner, 4.5)))[0]
        assert none is None and np.array_equal(b_pos.cpu().numpy(), want) and np.array_equal(want, by_path(want)) and len(want) > 300
        c.clear_voxels_device(b_pos)
        for p in want.tolist():
            scene.pop(tuple(p), None)
        assert 300 < len(scene) < 400
        g_pos, g_mrgb = c.get_voxels()
        keys = sorted(scene, key=S.path_key)
        assert np.array_equal(g_pos, np.array(keys, np.int16)) and np.array_equal(g_mrgb, np.array([scene[k] for k in keys], np.uint8))
        # a beam through it, from outside to outside
        a, b = (float(lo[0]) - 3, float(lo[1]) + 2.5, float(lo[2]) + 4.5), (float(hi[0]) + 2, float(hi[1]) - 1.5, float(hi[2]) + 3)
        k_pos, k_mrgb = c.capsule_voxels(a, b, 1.25, (0x83, 200, 40, 10))
        want_pos, want_mrgb = S.shape(*S.unpack(H, H.capsule_shape(a, b, 1.25)), (0x83, 200, 40, 10))
        assert np.array_equal(k_pos.cpu().numpy(), want_pos) and np.array_equal(k_mrgb.cpu().numpy(), want_mrgb) and len(want_pos) > 50
        c.edit_voxels_device(k_pos, k_mrgb, grow=True)
        scene.update({tuple(p): tuple(v) for p, v in zip(want_pos.tolist(), want_mrgb.tolist())})
        g_pos, g_mrgb = c.get_voxels()
        keys = sorted(scene, key=S.path_key)
        assert np.array_equal(g_pos, np.array(keys, np.int16)) and np.array_equal(g_mrgb, np.array([scene[k] for k in keys], np.uint8))
        # the result as a scene of its own, rendered
        e_pos, e_mrgb = c.ellipsoid_voxels((0, 0, 0), (5, 9, 14), None, (0, 0xB0, 0xD0, 0x60))
        c.set_voxels_device(e_pos, e_mrgb)
        assert c.count_voxels() == len(e_pos) > 2000
        s_pos, s_mrgb = c.get_voxels_device()
        assert torch.equal(s_pos, e_pos) and torch.equal(s_mrgb, e_mrgb)         # already in the scene's order
        c.camera = H.Camera((0.0, 0.0, -40.0), (0.0, 0.0, 1.0))
        c.render(H.ALL)
        image = c.read(H.SAMPLED_COLOR)
        assert image.shape[:2] == (64, 64)
