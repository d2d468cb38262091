"""GPU: vxrt_mesh_voxels_device (include/vxrt_mesh.h) against its rule in Python (tests/mesh_model.py).

Every case climbs one ladder (check): the count-only form with and without caps, two filling calls that write the same bytes between
intact guard bytes, both inputs unchanged, vertices, triangles and bytes equal to the model's bit for bit, the wrapper counting first
and with room to spare, and — where no coordinate is 32767 — the way back: the solid voxeliser's interior of the mesh is the set."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import mesh_model as MM
import solid_model as S
from list_op_harness import DEV, Bytes, by_path, last_error, on_device

pytestmark = pytest.mark.gpu

FILL = (7, 1, 2, 3)


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def raw(ctx, pos, mrgb, n, mode, verts, vert_cap, tris, tri_mrgb, tri_cap, given=(True, True)):
    """The C call over raw addresses -> (status, *n_verts, *n_tris)."""
    torch.cuda.synchronize()
    v, t = C.c_size_t(0xDEAD), C.c_size_t(0xBEEF)
    rc = ctx._L.vxrt_mesh_voxels_device(ctx._h, pos, mrgb, C.c_size_t(n), C.c_uint32(mode), verts, C.c_size_t(vert_cap), tris, tri_mrgb,
                                        C.c_size_t(tri_cap), C.byref(v) if given[0] else None, C.byref(t) if given[1] else None)
    return rc, v.value, t.value


def check(ctx, pos, mrgb, mode, what, shift=0, round_trip=None, want=None):
    """A list and a mode through every form of the call against the model -> (verts, tris, tri_mrgb) of the result.  The inputs and
    out_tri_mrgb start `shift` bytes past a 16-byte boundary, out_verts and out_tris 4 * shift (mod 16) bytes past one.  want: the
    model's result, where the caller has it already."""
    what = f"{what}: {MM.NAMES[mode]}"
    pos = np.ascontiguousarray(pos, np.int16).reshape(-1, 3)
    mrgb = None if mrgb is None else np.ascontiguousarray(mrgb, np.uint8).reshape(-1, 4)
    want_verts, want_tris, want_mrgb = MM.mesh(pos, mrgb, mode) if want is None else want
    nv, nt, n = len(want_verts), len(want_tris), len(pos)
    assert nv <= 8 * n and nt <= 12 * n
    aligned = 4 * shift % 16
    ins = [Bytes(pos.nbytes, shift, pos), None if mrgb is None else Bytes(mrgb.nbytes, shift, mrgb)]
    ptr = [None if b is None else b.ptr for b in ins]
    assert raw(ctx, *ptr, n, mode, None, 0, None, None, 0) == (0, nv, nt), (what, "count only", last_error(ctx))
    assert raw(ctx, *ptr, n, mode, None, 12345, None, None, 777) == (0, nv, nt), (what, "count only ignores the caps")
    outs = []
    for turn in range(2):
        out = [Bytes(12 * nv, aligned), Bytes(12 * nt, aligned), None if mrgb is None else Bytes(4 * nt, shift)]
        assert raw(ctx, *ptr, n, mode, out[0].ptr, nv, out[1].ptr, None if out[2] is None else out[2].ptr, nt) == (0, nv, nt), (what, f"call {turn}", last_error(ctx))
        assert all(b is None or b.guards_hold() for b in out), f"{what}: guard bytes"
        outs.append(out)
    for a, b in zip(*outs):
        assert a is None or a.all().tobytes() == b.all().tobytes(), f"{what}: a second call"
    for b, (name, v) in zip(ins, (("pos", pos), ("mrgb", mrgb))):
        assert b is None or (b.guards_hold() and b.data().tobytes() == v.tobytes()), f"{what}: {name} was written"
    got_verts = outs[0][0].data().view(np.float32).reshape(-1, 3)
    got_tris = outs[0][1].data().view(np.uint32).reshape(-1, 3)
    got_mrgb = None if mrgb is None else outs[0][2].data().reshape(-1, 4)
    assert got_verts.tobytes() == want_verts.tobytes(), f"{what}: {int((got_verts != want_verts).any(axis=1).sum())} of {nv} vertices differ"
    assert np.array_equal(got_tris, want_tris), f"{what}: {int((got_tris != want_tris).any(axis=1).sum())} of {nt} triangles differ"
    assert mrgb is None or np.array_equal(got_mrgb, want_mrgb), f"{what}: the triangles' bytes"
    # the wrapper, counting first and with room to spare
    dev = [on_device(pos), None if mrgb is None else on_device(mrgb)]
    for cap in (None, (nv + 3, nt + 5)):
        w_verts, w_tris, w_mrgb = ctx.mesh_voxels(*dev, mode, cap=cap)
        assert w_verts.dtype == torch.float32 and w_verts.device == DEV and tuple(w_verts.shape) == (nv, 3), what
        assert w_tris.dtype == torch.int32 and w_tris.device == DEV and tuple(w_tris.shape) == (nt, 3), what
        assert w_verts.cpu().numpy().tobytes() == want_verts.tobytes() and np.array_equal(w_tris.cpu().numpy().view(np.uint32), want_tris), f"{what}: the wrapper"
        assert (w_mrgb is None) == (mrgb is None)
        if mrgb is not None:
            assert w_mrgb.dtype == torch.uint8 and tuple(w_mrgb.shape) == (nt, 4) and np.array_equal(w_mrgb.cpu().numpy(), want_mrgb), f"{what}: the wrapper"
    # the way back: the inside of the mesh is the set
    if round_trip is None:
        round_trip = n > 0 and int(pos.max()) < 32767
    if round_trip:
        back, fill = ctx.voxelize_solid(w_verts, w_tris, None, FILL, interior_only=True)
        assert np.array_equal(back.cpu().numpy(), by_path(pos)), f"{what}: the interior of the mesh is not the set"
        assert len(fill) == len(back) and set(map(tuple, fill.cpu().numpy().tolist())) == {FILL}
        union, _ = ctx.voxelize_solid(w_verts, w_tris, (1, 2, 3, 4) if w_mrgb is None else w_mrgb, FILL)      # does not refuse
        assert len(union) >= len(back)
    return got_verts, got_tris, got_mrgb


def check_modes(ctx, pos, mrgb, what, shift=0):
    """Both modes -> the triangles of each."""
    return [len(check(ctx, pos, mrgb, mode, what, shift)[1]) for mode in MM.MODES]


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(32, 32) as c:      # no scene is loaded: the call needs none
        yield c


# ---- the smallest cases ------------------------------------------------------------------------------------------------------------
def test_nothing_and_one_voxel(H, ctx):
    one, red = MM.cells((3, -4, 5)), np.array([[0x85, 1, 2, 3]], np.uint8)
    assert check_modes(ctx, one[:0], red[:0], "nothing") == [0, 0]
    assert check_modes(ctx, one[:0], None, "nothing, positions only") == [0, 0]
    # an empty list touches no device pointer
    for mode in MM.MODES:
        assert raw(ctx, C.c_void_p(8), C.c_void_p(3), 0, mode, C.c_void_p(4), 4, C.c_void_p(12), C.c_void_p(7), 4) == (0, 0, 0)
    assert raw(ctx, None, None, 0, MM.RUNS, None, 0, None, None, 0) == (0, 0, 0)
    for shift in (0, 1, 3, 7):
        assert check_modes(ctx, one, red, "one voxel", shift) == [12, 12]
    verts, _, mrgb = check(ctx, one, red, MM.RUNS, "bit 7 goes")
    assert len(verts) == 8 and set(map(tuple, mrgb.tolist())) == {(5, 1, 2, 3)}
    assert check_modes(ctx, one, None, "one voxel, positions only", 5) == [12, 12]


def test_the_last_entry_of_a_position_wins(H, ctx):
    pos = MM.cells((1, 2, 3), (1, 2, 4), (1, 2, 3), (1, 2, 4), (1, 2, 3))
    mrgb = np.array([[0x81, 1, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [0xFF, 4, 5, 6], [0xFF, 4, 5, 6]], np.uint8)
    assert check_modes(ctx, pos, mrgb, "duplicates in other colours") == [20, 16]       # both voxels end as (0x7f, 4, 5, 6): the x-normal faces run
    mrgb[4] = (9, 9, 9, 9)
    assert check_modes(ctx, pos, mrgb, "duplicates in other colours") == [20, 20]       # now they differ: the runs along z break
    assert check_modes(ctx, pos, None, "duplicates, positions only", 3) == [20, 16]


def test_pairs_and_the_block_with_a_cavity(H, ctx):
    for name, pos in MM.small_families()[1:5]:
        for what, mrgb in (("positions only", None), ("one colour", MM.one_colour(len(pos))), ("three colours", MM.three_colours(len(pos), 4))):
            faces, runs = check_modes(ctx, pos, mrgb, f"{name}, {what}", shift=1)
            assert runs <= faces
    assert check_modes(ctx, MM.cavity(), None, "the cavity's faces") == [2 * (54 + 6), 2 * (6 * 3 + 6)]


def test_the_ends_of_the_int16_range(H, ctx):
    for axis in range(3):
        for at in (-32768, 32767):
            one = np.zeros((1, 3), np.int16)
            one[0, axis] = at
            assert check_modes(ctx, one, MM.one_colour(1), f"one voxel at {at} on axis {axis}", shift=3) == [12, 12]
            pair = np.zeros((2, 3), np.int16)
            pair[:, axis] = (at, at + 1) if at < 0 else (at - 1, at)
            assert check_modes(ctx, pair, MM.three_colours(2, axis), f"a pair ending at {at} on axis {axis}")[0] == 20
    corners = np.array([[x, y, z] for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)], np.int16)
    verts, _, _ = check(ctx, corners, MM.three_colours(8, 9), MM.RUNS, "all eight corners")
    assert verts.min() == -32768.0 and verts.max() == 32768.0 and len(verts) == 64
    # a run does not go on from the end of one row to the start of the next
    rows = MM.cells((0, 0, 32767), (0, 1, -32768), (32767, 5, 0), (-32768, 5, 1), (4, 32767, 4), (5, -32768, 4))
    assert check_modes(ctx, rows, None, "one row's end and the next row's start") == [72, 72]
    assert check_modes(ctx, rows, MM.one_colour(6), "one row's end and the next row's start", shift=7) == [72, 72]
    low = MM.cells((-32768, -32768, -32768), (-32768, -32768, -32767), (-32767, -32768, -32768))
    check_modes(ctx, low, MM.three_colours(3, 2), "the least corner: its mesh goes back through the solid voxeliser")


# ---- runs, blocks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_bar_of_3000(H, ctx, axis):
    # the two faces whose runs follow the bar give one quad each, 3 000 faces long, across the 2 048-entry blocks of the sorted faces;
    # the other two long sides give 3 000 one-cell quads each
    bar = MM.bar(axis)
    assert check_modes(ctx, bar, MM.one_colour(3000), f"a bar along axis {axis}") == [2 * (4 * 3000 + 2), 2 * (2 + 2 * 3000 + 2)]
    assert check_modes(ctx, bar[np.random.default_rng(axis).permutation(3000)], None, f"a shuffled bar along axis {axis}", shift=1)[1] == 2 * (2 + 2 * 3000 + 2)


@pytest.mark.parametrize("at", [2047, 2048])
def test_a_colour_change_beside_a_block_boundary(H, ctx, at):
    # along z the -x faces are the first 3 000 sorted faces, in the bar's order: sorted face `at` begins the second quad, as the last
    # entry of block 0 (2 047) or the first of block 1 (2 048), where it is compared with the last entry of the block before
    bar = MM.bar(2)
    mrgb = MM.one_colour(3000)
    mrgb[at:] = (6, 1, 1, 1)
    assert check_modes(ctx, bar, mrgb, f"a bar whose colour changes at {at}") == [2 * (4 * 3000 + 2), 2 * (4 + 2 * 3000 + 2)]
    mrgb[at:, 0] = 5 | 0x80
    mrgb[at:, 1:] = mrgb[0, 1:]
    assert check(ctx, bar, mrgb, MM.RUNS, "bit 7 does not end a run", round_trip=False)[1].shape[0] == 2 * (2 + 2 * 3000 + 2)


def test_a_random_list_of_2049(H, ctx):
    rng = np.random.default_rng(33)
    g = MM.block(-9, 9)                                   # 18^3 = 5 832 cells
    pos = g[rng.choice(len(g), 2049, replace=False)]
    faces, runs = check_modes(ctx, pos, MM.three_colours(2049, 34), "2 049 random cells", shift=3)
    assert runs < faces
    extra = np.concatenate([pos, pos[rng.integers(0, 2049, 100)]])      # 100 listed again, in other colours
    check_modes(ctx, extra, MM.three_colours(len(extra), 35), "... with duplicates")


def test_a_slab_in_three_colours(H, ctx):
    slab = MM.block((-20, -20, 0), (20, 20, 2))
    assert len(slab) == 3200
    faces, runs = check_modes(ctx, slab, MM.three_colours(3200, 36), "the slab")
    assert faces == 2 * (2 * 1600 + 4 * 80) and runs < faces
    # positions only on the same layout: runs merge across the colours
    f2, r2 = check_modes(ctx, slab, None, "the slab, positions only", shift=1)
    assert f2 == faces and r2 < runs and r2 == 2 * (2 * 40 + 2 * 40 + 2 * 2)


def test_a_torus_goes_round(H, ctx):
    (verts, tris), _, inner = S.table()["torus"]
    solid, fill = ctx.voxelize_solid(verts, tris, None, FILL, interior_only=True)
    assert len(solid) == inner
    for mode in (H.MESH_FACES, H.MESH_RUNS):
        m_verts, m_tris, m_mrgb = ctx.mesh_voxels(solid, fill, mode)
        assert len(m_tris) == len(m_mrgb) and 0 < len(m_verts) <= 8 * inner
        back, _ = ctx.voxelize_solid(m_verts, m_tris, m_mrgb, FILL, interior_only=True)
        assert torch.equal(back, solid), mode
        assert MM.volume6(m_verts.cpu().numpy(), m_tris.cpu().numpy()) == 6 * inner
    check_modes(ctx, solid.cpu().numpy(), fill.cpu().numpy(), "the torus")


# ---- room, aliasing, refusals ------------------------------------------------------------------------------------------------------
def test_the_bytes_may_go_where_the_inputs_bytes_are(H, ctx):
    pos = MM.block(-8, 8)
    mrgb = MM.one_colour(len(pos))
    want = MM.mesh(pos, mrgb, MM.RUNS)
    nv, nt = len(want[0]), len(want[1])
    assert nt == 2 * 6 * 16 and nt < len(pos)
    io = Bytes(mrgb.nbytes, 1, mrgb)
    d_pos, verts, tris = on_device(pos), Bytes(12 * nv), Bytes(12 * nt)
    assert raw(ctx, C.c_void_p(d_pos.data_ptr()), io.ptr, len(pos), MM.RUNS, verts.ptr, nv, tris.ptr, io.ptr, len(pos)) == (0, nv, nt), last_error(ctx)
    assert io.guards_hold() and verts.guards_hold() and tris.guards_hold()
    assert np.array_equal(io.data()[:4 * nt].reshape(-1, 4), want[2]) and io.data()[4 * nt:].tobytes() == mrgb.tobytes()[4 * nt:]
    assert verts.data().tobytes() == want[0].tobytes() and np.array_equal(tris.data().view(np.uint32).reshape(-1, 3), want[1])


def test_refusals_write_nothing(H, ctx):
    pos = MM.block(-4, 4)
    mrgb = MM.three_colours(len(pos), 40)
    n = len(pos)
    nv, nt = (len(a) for a in MM.mesh(pos, mrgb, MM.RUNS)[:2])
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    p, c = C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr())
    verts, tris, bytes_ = Bytes(12 * 8 * n), Bytes(12 * 12 * n), Bytes(4 * 12 * n)
    v, t, b, vroom, troom = verts.ptr, tris.ptr, bytes_.ptr, 8 * n, 12 * n

    def refused(*args, status=H.E_INVALID, says=None, counts=(0xDEAD, 0xBEEF), **kw):
        assert raw(ctx, *args, **kw) == (status, *counts), args
        assert last_error(ctx) and (says is None or says in last_error(ctx)), last_error(ctx)
        assert "vxrt_mesh_voxels_device" in last_error(ctx)
        assert verts.untouched() and tris.untouched() and bytes_.untouched()

    refused(p, c, 1 << 32, MM.RUNS, v, vroom, t, b, troom, says="2^32")                  # before any pointer is looked at
    refused(None, None, 1 << 32, 9, v, 0, None, None, 0, says="2^32", given=(False, False))
    refused(p, c, n, MM.RUNS, v, vroom, t, b, troom, says="n_verts", given=(False, True))
    refused(p, c, n, MM.RUNS, v, vroom, t, b, troom, says="n_tris", given=(True, False))
    for mode in (2, 3, 0xFFFFFFFF):
        refused(p, c, n, mode, v, vroom, t, b, troom, says="vxrt_mesh_mode")
    refused(p, c, n, 2, v, vroom, None, b, troom, says="vxrt_mesh_mode")                 # in the header's order
    for mode in MM.MODES:
        refused(p, c, n, mode, v, vroom, None, None, troom, says="out_verts and out_tris")
        refused(p, c, n, mode, None, vroom, t, b, troom, says="out_verts and out_tris")
        refused(p, None, n, mode, v, vroom, t, b, troom, says="out_tri_mrgb without mrgb")
        refused(p, None, n, mode, None, vroom, None, b, troom, says="out_tri_mrgb without mrgb")
        refused(p, c, n, mode, v, vroom, t, None, troom, says="out_tris and out_tri_mrgb")
        refused(p, c, n, mode, None, vroom, None, b, troom, says="out_tris and out_tri_mrgb")
    refused(None, c, n, MM.RUNS, v, vroom, t, b, troom, says="null voxel positions")
    # host memory, pageable and pinned
    refused(C.c_void_p(pos.ctypes.data), c, n, MM.RUNS, v, vroom, t, b, troom, says="pos")
    assert "not device memory" in last_error(ctx)
    pinned = torch.as_tensor(np.array(mrgb)).pin_memory()
    refused(p, C.c_void_p(pinned.data_ptr()), n, MM.RUNS, v, vroom, t, b, troom, says="mrgb")
    host = [np.zeros((vroom, 3), np.float32), np.zeros((troom, 3), np.uint32), np.zeros((troom, 4), np.uint8)]
    h = [C.c_void_p(a.ctypes.data) for a in host]
    refused(p, c, n, MM.RUNS, h[0], vroom, t, b, troom, says="out_verts")
    refused(p, c, n, MM.RUNS, v, vroom, h[1], b, troom, says="out_tris")
    refused(p, c, n, MM.RUNS, v, vroom, t, h[2], troom, says="out_tri_mrgb")
    assert not any(a.any() for a in host)
    # misaligned: out_verts and out_tris are arrays of 4-byte words
    for off in (1, 2, 3):
        refused(p, c, n, MM.RUNS, C.c_void_p(v.value + off), vroom - 1, t, b, troom, says="out_verts is not 4-byte aligned")
        refused(p, c, n, MM.RUNS, v, vroom, C.c_void_p(t.value + off), b, troom - 1, says="out_tris is not 4-byte aligned")
    # an output one entry short of its cap: an allocation of its own, because what the library can see is the allocation
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    cap = 1025                                                                      # 1024 entries of 4 bytes are a whole page: no rounding hides the missing one
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (cap - 1))) == 0
    refused(p, c, n, MM.RUNS, v, vroom, t, short, cap, says="past its allocation")
    assert "out_tri_mrgb" in last_error(ctx)
    assert hip.hipFree(short) == 0
    # room for one vertex or one triangle too few: both counts are set, nothing is written
    refused(p, c, n, MM.RUNS, v, nv - 1, t, b, nt, says=str(nv), counts=(nv, nt))
    assert str(nv - 1) in last_error(ctx) and str(nt) in last_error(ctx)
    refused(p, c, n, MM.RUNS, v, nv, t, b, nt - 1, says=str(nt - 1), counts=(nv, nt))
    refused(p, c, n, MM.RUNS, v, 0, t, b, 0, counts=(nv, nt))
    with pytest.raises(H.VxrtError) as e:
        ctx.mesh_voxels(d_pos, d_mrgb, H.MESH_RUNS, cap=(nv - 1, nt))
    assert e.value.status == H.E_INVALID
    with pytest.raises(H.VxrtError) as e:
        ctx.mesh_voxels(d_pos, d_mrgb, H.MESH_RUNS, cap=(nv, nt - 1))
    assert e.value.status == H.E_INVALID
    with pytest.raises(H.VxrtError) as e:                                            # no room at all is no counting call
        ctx.mesh_voxels(d_pos, d_mrgb, H.MESH_RUNS, cap=(0, 0))
    assert e.value.status == H.E_INVALID
    # ... and the valid call is accepted afterwards, at exactly the counts
    assert raw(ctx, p, c, n, MM.RUNS, v, nv, t, b, nt) == (0, nv, nt) and verts.guards_hold() and tris.guards_hold() and bytes_.guards_hold()
    assert np.array_equal(d_pos.cpu().numpy(), pos) and np.array_equal(d_mrgb.cpu().numpy(), mrgb)
