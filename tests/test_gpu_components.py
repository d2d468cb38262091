"""GPU: the connected components of a device voxel list and the detached voxels of a loaded scene (include/vxrt_components.h).  Every
comparison is bit for bit against the model of the rule (components_model.py): labels and count for connectivity 6, 18 and 26, and
for the scene call positions, bytes, order and count.  Every labelling also checks that guard words before and after `label` stay
untouched, that `pos` is unchanged, that a second call writes identical bytes and that the count-only form gives the same count.

The serpentine cases come twice.  Listed cell by cell through a 16^3 or 32^3 cube the path visits every cell, so the voxels form a
solid cube, whose list order is the long path but whose graph is not; the same path drawn on a lattice of twice the pitch (the
cells at even coordinates, and the one cell between each two consecutive ones) is a chain in the graph as well, with a diameter of
8 190 and 65 534 steps at every connectivity, which is what a labelling whose launches depend on the diameter, or one that trusts
a stale parent, gets wrong."""
import ctypes as C
import functools

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import components_model as K
from test_gpu_device_build import assert_same_scene
from test_gpu_edit import make_ctx
from test_gpu_voxelize import CFG, DEV, GUARD_MRGB, guarded, on_device, untouched

pytestmark = pytest.mark.gpu

GUARD = 0x5A5AA5A5
GUARD_WORDS = 8
MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)


@pytest.fixture(scope="module")
def ctx(H):
    with make_ctx(H, CFG) as c:      # no scene is loaded: the labelling needs none
        yield c


def ptr(a):
    if a is None or isinstance(a, C.c_void_p):
        return a
    return C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a)


def raw_label(ctx, pos, n, connectivity, label):
    """The C call over device tensors / raw addresses -> (status, *n_components)."""
    got = C.c_size_t(0xDEAD)
    rc = ctx._L.vxrt_label_components_device(ctx._h, ptr(pos), C.c_size_t(n), C.c_uint32(connectivity), ptr(label), C.byref(got))
    return rc, got.value


def raw_detached(ctx, lo, hi, connectivity, pos, out, cap):
    got = C.c_size_t(0xDEAD)
    box = [None if b is None else (C.c_int32 * 3)(*[int(v) for v in b]) for b in (lo, hi)]
    rc = ctx._L.vxrt_detached_voxels_device(ctx._h, box[0], box[1], C.c_uint32(connectivity), ptr(pos), ptr(out), C.c_size_t(cap), C.byref(got))
    return rc, got.value


def last_error(ctx):
    return (ctx._L.vxrt_last_error() or b"").decode()


def guarded_label(n):
    buf = torch.full((n + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    return buf


def guards_hold(buf, n):
    words = buf.cpu().numpy().view(np.uint32)
    return bool((words[:GUARD_WORDS] == GUARD).all()) and bool((words[GUARD_WORDS + n:] == GUARD).all())


def labelled(ctx, d_pos, n, connectivity):
    """one guarded call -> (label uint32 [n], n_components)"""
    buf = guarded_label(n)
    rc, count = raw_label(ctx, d_pos if n else None, n, connectivity, C.c_void_p(buf.data_ptr() + 4 * GUARD_WORDS))
    assert rc == 0, last_error(ctx)
    assert guards_hold(buf, n), "the guard words around label"
    return buf.cpu().numpy().view(np.uint32)[GUARD_WORDS:GUARD_WORDS + n].copy(), count


def check(ctx, pos, want, what, connectivities=K.CONNECTIVITIES):
    """pos int16 [n, 3]; want: connectivity -> (label, count)"""
    pos = np.ascontiguousarray(pos, np.int16).reshape(-1, 3)
    n = len(pos)
    d_pos = on_device(pos)
    for conn in connectivities:
        label, count = labelled(ctx, d_pos, n, conn)
        again, count2 = labelled(ctx, d_pos, n, conn)
        assert count == count2 == want[conn][1], (what, conn, count, count2, want[conn][1])
        assert np.array_equal(label, want[conn][0]), (what, conn, "labels", int((label != want[conn][0]).sum()))
        assert label.tobytes() == again.tobytes(), (what, conn, "a second call")
        assert raw_label(ctx, d_pos if n else None, n, conn, None) == (0, count), (what, conn, "count only")
        assert np.array_equal(d_pos.cpu().numpy(), pos), (what, conn, "pos was written")


def modelled(pos):
    return {conn: K.label(pos, conn) for conn in K.CONNECTIVITIES}


def one_component(n):
    return {conn: (np.zeros(n, np.uint32), 1) for conn in K.CONNECTIVITIES}


# ---- the smallest lists ------------------------------------------------------------------------------------------------------------
def test_lists_of_none_one_and_two(ctx, H):
    check(ctx, np.zeros((0, 3), np.int16), {c: (np.zeros(0, np.uint32), 0) for c in K.CONNECTIVITIES}, "n = 0")
    check(ctx, [[7, -9, 11]], one_component(1), "n = 1")
    check(ctx, [[7, -9, 11], [7, -9, 11]], one_component(2), "n = 2, one position")
    check(ctx, [[7, -9, 11], [-7, 9, -11]], {c: (np.array([0, 1], np.uint32), 2) for c in K.CONNECTIVITIES}, "n = 2, apart")
    # the wrapper: the same labels as a uint32 tensor, a numpy list uploaded first
    label, count = ctx.label_components(np.array([[0, 0, 0], [5, 5, 5], [0, 1, 0]], np.int16))
    assert label.dtype == torch.uint32 and label.device == DEV and (label.cpu().numpy().tolist(), count) == ([0, 1, 0], 2)
    label, count = ctx.label_components(torch.zeros((0, 3), dtype=torch.int16, device=DEV), 26)
    assert tuple(label.shape) == (0,) and count == 0
    label, count = ctx.label_components(on_device(np.array([[0, 0, 0], [1, 1, 1]], np.int16)), connectivity=26)
    assert (label.cpu().numpy().tolist(), count) == ([0, 0], 1)


PAIRS = {"face": ((3, 4, 5), (3, 5, 5), [1, 1, 1]), "edge": ((3, 4, 5), (4, 5, 5), [2, 1, 1]), "corner": ((3, 4, 5), (4, 3, 6), [2, 2, 1]),
         "wrap": ((32767, 0, 0), (-32768, 0, 0), [2, 2, 2]), "wrap on every axis": ((32767, 32767, 32767), (-32768, -32768, -32768), [2, 2, 2]),
         "across the origin": ((-1, 0, 0), (0, 0, 0), [1, 1, 1]), "corner across the origin": ((-1, -1, -1), (0, 0, 0), [2, 2, 1])}


@pytest.mark.parametrize("name", list(PAIRS))
def test_adjacency_pairs(ctx, name):
    a, b, counts = PAIRS[name]
    for pair in ([a, b], [b, a]):
        want = {c: (np.array([0, 0] if k == 1 else [0, 1], np.uint32), k) for c, k in zip(K.CONNECTIVITIES, counts)}
        assert all(K.label(pair, c)[1] == want[c][1] for c in K.CONNECTIVITIES)
        check(ctx, pair, want, name)


def test_duplicates_and_order(ctx):
    rng = np.random.default_rng(11)
    cells = np.unique(rng.integers(-6, 7, (600, 3)), axis=0)
    cells = cells[rng.permutation(len(cells))[:300]]
    assert len(cells) == 300
    pos = np.repeat(cells, rng.integers(1, 5, 300), axis=0)
    pos = pos[rng.permutation(len(pos))]
    want = modelled(pos)
    assert 1 < want[6][1] < 300 and (want[6][0] <= np.arange(len(pos))).all()
    check(ctx, pos, want, "duplicates")


@pytest.mark.parametrize("n", [255, 256, 257, 2047, 2048, 2049, 4097])
def test_separated_runs_along_x(ctx, n):
    lengths = [63, 64, 65, 255, 256, 257, 1, 2]      # they straddle a wave and a block
    pos, x, k = [], -3000, 0
    while len(pos) < n:
        run = min(lengths[k % len(lengths)], n - len(pos))
        pos += [(x + i, 5, -5) for i in range(run)]
        x += run + 1                                  # one empty cell between two runs
        k += 1
    pos = np.array(pos, np.int16)
    first = np.concatenate([[0], np.nonzero(np.diff(pos[:, 0]) != 1)[0] + 1])
    label = np.repeat(first, np.diff(np.concatenate([first, [n]]))).astype(np.uint32)
    want = {c: (label, len(first)) for c in K.CONNECTIVITIES}      # by hand: a run is labelled with its first index
    if n <= 2049:
        assert np.array_equal(K.label(pos, 6)[0], label)
    check(ctx, pos, want, f"runs, n = {n}")


# ---- long chains -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def serpentine(side):
    """the cells of side^3 along a path that turns back at the end of every row and of every layer: consecutive cells share a face"""
    out = []
    for z in range(side):
        for j in range(side):
            y = side - 1 - j if z % 2 else j
            row = z * side + j
            out += [((side - 1 - i if row % 2 else i), y, z) for i in range(side)]
    path = np.array(out, np.int64)
    assert (np.abs(np.diff(path, axis=0)).sum(axis=1) == 1).all() and len(np.unique(path, axis=0)) == side ** 3
    path.setflags(write=False)
    return path


@functools.lru_cache(maxsize=None)
def chain(side):
    """the same path at twice the pitch with the cell between each two consecutive ones: 2 side^3 - 1 voxels, each touching only its
    neighbours along the path (and, by a corner or an edge, the next but one at a turn)"""
    path = 2 * serpentine(side)
    out = np.empty((2 * len(path) - 1, 3), np.int64)
    out[0::2] = path
    out[1::2] = (path[1:] + path[:-1]) // 2
    out -= side
    out.setflags(write=False)
    return out


def orders(pos, seed):
    return {"head first": pos, "tail first": pos[::-1], "shuffled": pos[np.random.default_rng(seed).permutation(len(pos))]}


@pytest.mark.parametrize("order", ["head first", "tail first", "shuffled"])
@pytest.mark.parametrize("side", [16, 32])
@pytest.mark.parametrize("shape", ["cube", "chain"])
def test_serpentines(ctx, shape, side, order):
    pos = orders(serpentine(side) - side // 2 if shape == "cube" else chain(side), side)[order]
    assert len(pos) == (side ** 3 if shape == "cube" else 2 * side ** 3 - 1)
    if side == 16 and order == "shuffled":
        want = modelled(pos)
        assert all(want[c][1] == 1 and not want[c][0].any() for c in K.CONNECTIVITIES)
    check(ctx, pos, one_component(len(pos)), f"{shape} {side} {order}")      # one component: every label is the least index, 0


def test_a_chain_cut_in_the_middle(ctx):
    pos = chain(16)
    cut = len(pos) // 2
    pos = np.delete(pos, [cut - 1, cut, cut + 1], axis=0)      # three cells: the diagonal at a turn cannot bridge it
    shuffled = pos[np.random.default_rng(5).permutation(len(pos))]
    want = modelled(shuffled)
    assert [want[c][1] for c in K.CONNECTIVITIES] == [2, 2, 2]
    check(ctx, shuffled, want, "cut chain")


# ---- many merges -------------------------------------------------------------------------------------------------------------------
def combs():
    """Two combs in 32 x 32 x 2 whose teeth interleave without touching, joined by a bridge in the second layer at x = 31 only"""
    a = [(x, 0, 0) for x in range(32)] + [(x, y, 0) for x in range(0, 32, 4) for y in range(1, 30)]
    b = [(x, 31, 0) for x in range(32)] + [(x, y, 0) for x in range(2, 32, 4) for y in range(2, 31)]
    bridge = [(31, y, 1) for y in range(32)]
    return np.array(a, np.int64), np.array(b, np.int64), np.array(bridge, np.int64)


def test_two_combs_joined_at_one_end(ctx):
    a, b, bridge = combs()
    apart = modelled(np.concatenate([a, b]))
    assert [apart[c][1] for c in K.CONNECTIVITIES] == [2, 2, 2]
    for seed in (0, 1):
        pos = np.concatenate([a, b, bridge])
        if seed:
            pos = pos[np.random.default_rng(seed).permutation(len(pos))]
        want = modelled(pos)
        assert [want[c][1] for c in K.CONNECTIVITIES] == [1, 1, 1]
        check(ctx, pos, want, f"combs {seed}")
    check(ctx, np.concatenate([b, a]), modelled(np.concatenate([b, a])), "combs apart")


def test_checkerboard(ctx):
    board = np.argwhere(np.indices((16, 16, 16)).sum(axis=0) % 2 == 0) - 8
    want = {6: (np.arange(2048, dtype=np.uint32), 2048), 18: (np.zeros(2048, np.uint32), 1), 26: (np.zeros(2048, np.uint32), 1)}
    check(ctx, board, want, "checkerboard")
    shuffled = board[np.random.default_rng(3).permutation(2048)]
    check(ctx, shuffled, want, "checkerboard, shuffled")


# ---- random grids around the percolation threshold --------------------------------------------------------------------------------------
RANDOM = {1: 0.25, 2: 0.31, 3: 0.40}


@functools.lru_cache(maxsize=None)
def random_list(seed):
    """-> (cells int64 [n, 3] in [0, 40)^3, shuffled, 5 % of them listed twice; the model's labels per connectivity)"""
    rng = np.random.default_rng(seed)
    cells = np.argwhere(rng.random((40, 40, 40)) < RANDOM[seed])
    cells = np.concatenate([cells, cells[rng.integers(0, len(cells), len(cells) // 20)]])
    cells = cells[rng.permutation(len(cells))]
    cells.setflags(write=False)
    return cells, modelled(cells)


@pytest.mark.parametrize("seed", list(RANDOM))
def test_random_grids(ctx, seed):
    cells, want = random_list(seed)
    sizes = np.bincount(want[6][0])
    assert want[6][1] > 1000 and (sizes.max() < 500 if seed == 1 else sizes.max() > 1000)      # below the threshold: small ones only;
    assert seed != 3 or sizes.max() > 20000                                                    # above it: a giant one beside them
    assert want[6][1] > want[18][1] > want[26][1] >= 1
    check(ctx, cells - 20, want, f"seed {seed}, around the origin")
    far = cells + (32768 - 40)
    assert far.max() == 32767
    if seed == 1:
        assert all(np.array_equal(K.label(far, c)[0], want[c][0]) for c in (6, 26))      # the model itself does not care where the box lies
    check(ctx, far, want, f"seed {seed}, ending at 32767")


def test_a_list_at_an_odd_address(ctx):
    cells, want = random_list(1)
    pos = np.ascontiguousarray(cells[:3001] - 20, np.int16)
    expect = modelled(pos)
    raw = torch.zeros(pos.nbytes + 8, dtype=torch.uint8, device=DEV)
    for off in (1, 2, 3):
        raw[off:off + pos.nbytes] = torch.as_tensor(pos.view(np.uint8).reshape(-1), device=DEV)
        torch.cuda.synchronize()
        buf = guarded_label(len(pos))
        rc, count = raw_label(ctx, C.c_void_p(raw.data_ptr() + off), len(pos), 18, C.c_void_p(buf.data_ptr() + 4 * GUARD_WORDS))
        assert (rc, count) == (0, expect[18][1]) and guards_hold(buf, len(pos)), off
        assert np.array_equal(buf.cpu().numpy().view(np.uint32)[GUARD_WORDS:-GUARD_WORDS], expect[18][0]), off


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx, H):
    n = 1025
    pos = np.zeros((n, 3), np.int16)
    pos[:, 0] = np.arange(n)
    d_pos = on_device(pos)
    buf = guarded_label(n)
    label = C.c_void_p(buf.data_ptr() + 4 * GUARD_WORDS)

    def refused(*args):
        rc, count = raw_label(ctx, *args)
        assert rc == H.E_INVALID and count == 0xDEAD, (rc, count)
        assert last_error(ctx)
        assert (buf.cpu().numpy().view(np.uint32) == GUARD).all()

    for connectivity in (0, 7, 27):
        refused(d_pos, n, connectivity, label)
        refused(d_pos, n, connectivity, None)
    refused(C.c_void_p(pos.ctypes.data), n, 6, label)                     # host memory, pageable
    refused(torch.as_tensor(pos).pin_memory(), n, 6, label)               # ... and pinned
    refused(None, n, 6, label)
    refused(d_pos, n, 6, C.c_void_p(label.value + 2))                     # label misaligned by 2 bytes
    refused(d_pos, 1 << 32, 6, label)                                     # checked before any pointer is looked at
    refused(None, 1 << 32, 6, None)
    # a label array one entry short.  It is an allocation of its own, because what the library can see is the allocation: a torch
    # tensor lies in a larger block of torch's allocator.  1024 words are whole pages, so no rounding hides the missing entry
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (n - 1))) == 0
    refused(d_pos, n, 6, short)
    assert "label" in last_error(ctx) and last_error(ctx).startswith("vxrt_label_components_device:")     # the entry point that was called
    assert raw_label(ctx, d_pos, n - 1, 6, short) == (0, 1)               # it holds n - 1
    small = C.c_void_p()
    assert hip.hipMalloc(C.byref(small), C.c_size_t(6 * (n - 1))) == 0    # ... and a list one position short
    refused(small, n, 6, label)
    assert hip.hipFree(short) == 0 and hip.hipFree(small) == 0
    assert ctx._L.vxrt_label_components_device(ctx._h, ptr(d_pos), C.c_size_t(n), C.c_uint32(6), label, None) == H.E_INVALID
    assert (buf.cpu().numpy().view(np.uint32) == GUARD).all()
    # ... and the valid call is accepted afterwards
    assert raw_label(ctx, d_pos, n, 6, label) == (0, 1)
    assert guards_hold(buf, n) and not buf.cpu().numpy()[GUARD_WORDS:-GUARD_WORDS].any()


# ---- the scene call ------------------------------------------------------------------------------------------------------------------
def voxel_dict(pos, mrgb):
    return {tuple(p): tuple(b) for p, b in zip(np.asarray(pos).tolist(), np.asarray(mrgb).tolist())}


@pytest.fixture(scope="module")
def sponge(H):
    """the level-3 sponge as get_voxels gives it: (pos, mrgb, dict, anchor box = its lowest y layer, the y of the layer to clear)"""
    with make_ctx(H, CFG) as c:
        c.set_menger(3, 0, MENGER_MRGB)
        pos, mrgb = c.get_voxels()
    assert len(pos) == 8000
    lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
    anchor = (tuple(lo.tolist()), (int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))
    return pos, mrgb, voxel_dict(pos, mrgb), anchor, int(lo[1]) + 8


def assert_detached(ctx, anchor, conn, want, what):
    pos, mrgb = ctx.detached_voxels(*anchor, connectivity=conn)
    assert pos.device == DEV and pos.dtype == torch.int16 and mrgb.dtype == torch.uint8, what
    assert tuple(pos.shape) == (len(want[0]), 3) and tuple(mrgb.shape) == (len(want[0]), 4), (what, tuple(pos.shape), len(want[0]))
    assert np.array_equal(pos.cpu().numpy(), want[0]), f"{what}: positions"
    assert np.array_equal(mrgb.cpu().numpy(), want[1]), f"{what}: mrgb"
    assert raw_detached(ctx, *anchor, conn, None, None, 0) == (0, len(want[0])), f"{what}: count only"


def staircase(voxels, y):
    """(x, z) with the sponge solid at (x, y - 1, z), (x, y, z), (x + 1, y + 1, z + 1) and (x + 1, y + 2, z + 1): with the layers y
    and y + 1 cleared but for the two middle cells, the halves hang together by one corner"""
    for x, yy, z in sorted(voxels):
        if yy == y and all(c in voxels for c in ((x, y - 1, z), (x + 1, y + 1, z + 1), (x + 1, y + 2, z + 1))):
            return x, z
    raise AssertionError("no staircase")


@pytest.mark.parametrize("conn", [6, 26])
def test_detached_voxels_of_an_edited_sponge(H, sponge, conn):
    pos, mrgb, voxels, anchor, layer = sponge
    with make_ctx(H, CFG) as c:
        c.set_menger(3, 0, MENGER_MRGB)
        records = c.read_scene()
        assert_detached(c, anchor, conn, (pos[:0], mrgb[:0]), "untouched")
        empty = ((0, 0, 0), (0, 5, 5))
        assert_detached(c, empty, conn, (pos, mrgb), "an empty anchor box")
        assert_detached(c, ((100, 100, 100), (200, 200, 200)), conn, (pos, mrgb), "an anchor box that misses the scene")
        # one whole layer cleared: everything above it hangs in the air
        gone = pos[pos[:, 1] == layer]
        c.clear_voxels_device(on_device(gone))
        model = {p: b for p, b in voxels.items() if p[1] != layer}
        want = K.detached(model, *anchor, conn)
        assert len(want[0]) == int((pos[:, 1] > layer).sum()) > 3000
        after = c.read_scene()
        assert_detached(c, anchor, conn, want, "a layer cleared")
        for a, b in zip(c.read_scene(), after):
            assert np.array_equal(a, b), "the call changed the scene"
        # room for one voxel less: the count, an error and nothing written; odd addresses; exactly enough
        k = len(want[0])
        gp, gm = guarded(k + 2)
        assert raw_detached(c, *anchor, conn, gp, gm, k - 1) == (H.E_INVALID, k)
        assert last_error(c) == f"vxrt_detached_voxels_device: {k} voxels, room for {k - 1}"      # the entry point that was called
        assert untouched(gp, gm)
        assert raw_detached(c, *anchor, conn, gp, None, k)[0] == H.E_INVALID and raw_detached(c, None, anchor[1], conn, gp, gm, k)[0] == H.E_INVALID
        for bad in (0, 7, 27):
            assert raw_detached(c, *anchor, bad, gp, gm, k + 2) == (H.E_INVALID, 0xDEAD)
        assert untouched(gp, gm)
        assert raw_detached(c, *anchor, conn, gp, gm, k) == (0, k)
        assert np.array_equal(gp[:k].cpu().numpy(), want[0]) and np.array_equal(gm[:k].cpu().numpy(), want[1])
        assert untouched(gp[k:], gm[k:])
        bp = torch.full((6 * k + 8,), GUARD_MRGB, dtype=torch.uint8, device=DEV)
        bm = torch.full((4 * k + 8,), GUARD_MRGB, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        assert raw_detached(c, *anchor, conn, C.c_void_p(bp.data_ptr() + 1), C.c_void_p(bm.data_ptr() + 2), k) == (0, k)
        assert bp[1:1 + 6 * k].cpu().numpy().tobytes() == want[0].tobytes() and bm[2:2 + 4 * k].cpu().numpy().tobytes() == want[1].tobytes()
        assert bool((bp[:1] == GUARD_MRGB).all()) and bool((bp[1 + 6 * k:] == GUARD_MRGB).all())
        assert bool((bm[:2] == GUARD_MRGB).all()) and bool((bm[2 + 4 * k:] == GUARD_MRGB).all())
        # the same scene in treelet order, which the extract reads and the editor refuses
        with make_ctx(H, (1, 1, 1, 1), tuning=[(H.OPT_NODE_ORDER, 2)]) as t:
            t.recreate_octree(np.array(list(model), np.int16), np.array(list(model.values()), np.uint8))
            assert t.stats().node_order == 2
            assert_detached(t, anchor, conn, want, "treelet order")
        # drop_detached: the returned list is what was removed, and what is left is the model's remainder
        with make_ctx(H, CFG) as twin:
            twin.set_menger(3, 0, MENGER_MRGB)
            twin.clear_voxels_device(on_device(gone))
            twin.clear_voxels_device(on_device(want[0]))
            removed = c.drop_detached(*anchor, connectivity=conn)
            assert np.array_equal(removed[0].cpu().numpy(), want[0]) and np.array_equal(removed[1].cpu().numpy(), want[1])
            assert_same_scene(c, twin, "drop_detached against clearing the model's list")
        dropped = set(map(tuple, want[0].tolist()))
        left = {p: b for p, b in model.items() if p not in dropped}
        assert len(left) == 8000 - len(gone) - k and c.count_voxels() == len(left)
        assert_detached(c, anchor, conn, (pos[:0], mrgb[:0]), "nothing is left to drop")
        c.fit_scene_depth()
        c.compact_scene()
        with make_ctx(H, CFG) as ref:
            ref.recreate_octree(np.array(sorted(left), np.int16), np.array([left[p] for p in sorted(left)], np.uint8))
            assert ref.scene_depth == c.scene_depth
            assert_same_scene(c, ref, "drop_detached, fitted and compacted, against a fresh build of the remainder")
        assert len(records[0]) > len(c.read_scene()[0])


def test_a_staircase_holds_by_its_corners_only(H, sponge):
    pos, mrgb, voxels, anchor, layer = sponge
    x, z = staircase(voxels, layer)
    keep = {(x, layer, z), (x + 1, layer + 1, z + 1)}
    gone = np.array([p for p in voxels if p[1] in (layer, layer + 1) and p not in keep], np.int16)
    model = {p: b for p, b in voxels.items() if p[1] not in (layer, layer + 1) or p in keep}
    want = {conn: K.detached(model, *anchor, conn) for conn in K.CONNECTIVITIES}
    above = int((pos[:, 1] > layer + 1).sum())
    assert [len(want[conn][0]) for conn in K.CONNECTIVITIES] == [above + 1, above + 1, 0]      # the upper step falls with the upper half
    with make_ctx(H, CFG) as c:
        c.set_menger(3, 0, MENGER_MRGB)
        c.clear_voxels_device(on_device(gone))
        for conn in K.CONNECTIVITIES:
            assert_detached(c, anchor, conn, want[conn], f"staircase, {conn}")


def test_no_scene_and_an_empty_scene(ctx, H):
    with pytest.raises(H.VxrtError) as e:
        ctx.detached_voxels((0, 0, 0), (1, 1, 1))
    assert e.value.status == H.E_NOSCENE
    assert raw_detached(ctx, (0, 0, 0), (1, 1, 1), 6, None, None, 0) == (H.E_NOSCENE, 0xDEAD)
    with make_ctx(H, CFG) as c:
        c.recreate_octree(np.array([[1, 2, 3]], np.int16), np.array([[1, 2, 3, 4]], np.uint8))
        c.clear_voxels(np.array([[1, 2, 3]], np.int16))
        pos, mrgb = c.detached_voxels((0, 0, 0), (1, 1, 1))
        assert tuple(pos.shape) == (0, 3) and tuple(mrgb.shape) == (0, 4)
        assert tuple(c.drop_detached((0, 0, 0), (1, 1, 1))[0].shape) == (0, 3)
