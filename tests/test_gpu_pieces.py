"""GPU: the component table of a device voxel list and the detached pieces of a loaded scene (include/vxrt_pieces.h).  Every comparison
is for exact equality with the model of the rule (pieces_model.py on top of components_model.py): label, id, every field of every
vxrt_piece including reserved == 0, and the counts.  Every table case also checks guard words before and after each output array,
that `pos` is unchanged, that a second call writes the same bytes, that the count-only form agrees and that `label` holds
label_components' bytes.

Where the model would take many seconds (the chain of 65 535 voxels in three orders, the two blocks of 163 840 voxels) the labels
are known by hand, as in test_gpu_components.py, and the table comes from them by numpy (hand_table), which the smaller cases check
against the model first."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import components_model as K
import pieces_model as P
from test_gpu_components import chain, combs, random_list
from test_gpu_device_build import assert_same_scene
from test_gpu_edit import make_ctx
from test_gpu_voxelize import CFG, DEV, GUARD_MRGB, guarded, on_device, untouched

pytestmark = pytest.mark.gpu

GUARD = 0x5A5AA5A5
GUARD_WORDS = 8                      # 32 bytes: what follows stays 8-byte aligned
PIECE_WORDS = P.PIECE.itemsize // 4
MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)
EVERY = P.EVERY


@pytest.fixture(scope="module")
def ctx(H):
    with make_ctx(H, CFG) as c:      # no scene is loaded: the table needs none
        yield c


def ptr(a):
    if a is None or isinstance(a, C.c_void_p):
        return a
    return C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a)


def raw_table(ctx, pos, n, connectivity, label, ids, info, info_cap):
    """The C call over device tensors / raw addresses -> (status, *n_components)."""
    got = C.c_size_t(0xDEAD)
    rc = ctx._L.vxrt_component_table_device(ctx._h, ptr(pos), C.c_size_t(n), C.c_uint32(connectivity), ptr(label), ptr(ids), ptr(info),
                                            C.c_size_t(info_cap), C.byref(got))
    return rc, got.value


def raw_pieces(ctx, lo, hi, connectivity, min_voxels, max_voxels, pos, out, piece, cap, info, info_cap):
    """-> (status, *n, *n_pieces)"""
    got, pieces = C.c_size_t(0xDEAD), C.c_size_t(0xBEEF)
    box = [None if b is None else (C.c_int32 * 3)(*[int(v) for v in b]) for b in (lo, hi)]
    rc = ctx._L.vxrt_detached_pieces_device(ctx._h, box[0], box[1], C.c_uint32(connectivity), C.c_uint32(min_voxels), C.c_uint32(max_voxels),
                                            ptr(pos), ptr(out), ptr(piece), C.c_size_t(cap), C.byref(got), ptr(info), C.c_size_t(info_cap),
                                            C.byref(pieces))
    return rc, got.value, pieces.value


def last_error(ctx):
    return (ctx._L.vxrt_last_error() or b"").decode()


class Words:
    """n 32-bit words of device memory between guard words"""
    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * GUARD_WORDS)

    def all(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def guards_hold(self, used=None):
        words, used = self.all(), self.n if used is None else used
        return bool((words[:GUARD_WORDS] == GUARD).all()) and bool((words[GUARD_WORDS + used:] == GUARD).all())

    def untouched(self):
        return bool((self.all() == GUARD).all())

    def words(self, used=None):
        return self.all()[GUARD_WORDS:GUARD_WORDS + (self.n if used is None else used)].copy()

    def pieces(self, k):
        return self.words(k * PIECE_WORDS).view(P.PIECE)


def assert_tables_equal(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in P.FIELDS:
        assert np.array_equal(got[f], want[f]), (what, f, got[f][:4], want[f][:4])
    assert not got["reserved"].any(), (what, "reserved")


def tabled(ctx, d_pos, n, connectivity, k):
    """one guarded call with room for k records -> (label, id, table, n_components)"""
    label, ids, info = Words(n), Words(n), Words(k * PIECE_WORDS)
    rc, count = raw_table(ctx, d_pos if n else None, n, connectivity, label.ptr, ids.ptr, info.ptr, k)
    assert rc == 0, last_error(ctx)
    assert label.guards_hold() and ids.guards_hold() and info.guards_hold(), "the guard words around label, id and info"
    return label.words(), ids.words(), info.pieces(k), count


def check(ctx, pos, want, what, connectivities=K.CONNECTIVITIES):
    """pos int16 [n, 3]; want: connectivity -> (label, id, table)"""
    pos = np.ascontiguousarray(pos, np.int16).reshape(-1, 3)
    n = len(pos)
    d_pos = on_device(pos)
    for conn in connectivities:
        w_label, w_ids, w_table = want[conn]
        k = len(w_table)
        assert raw_table(ctx, d_pos if n else None, n, conn, None, None, None, 0) == (0, k), (what, conn, "count only")
        label, ids, table, count = tabled(ctx, d_pos, n, conn, k)
        assert count == k, (what, conn, count, k)
        assert np.array_equal(label, w_label), (what, conn, "labels", int((label != w_label).sum()))
        assert np.array_equal(ids, w_ids), (what, conn, "ids", int((ids != w_ids).sum()))
        assert_tables_equal(table, w_table, (what, conn))
        again = tabled(ctx, d_pos, n, conn, k)
        assert again[3] == k and all(a.tobytes() == b.tobytes() for a, b in zip((label, ids, table), again[:3])), (what, conn, "a second call")
        mere, mere_count = ctx.label_components(d_pos, conn)
        assert mere_count == k and mere.cpu().numpy().tobytes() == label.tobytes(), (what, conn, "label_components' bytes")
        assert np.array_equal(mere.cpu().numpy(), w_label), (what, conn, "label_components against the model")
        assert np.array_equal(d_pos.cpu().numpy(), pos), (what, conn, "pos was written")


def modelled(pos):
    return {conn: P.component_table(pos, conn) for conn in K.CONNECTIVITIES}


def hand_table(pos, label):
    """(label, id, table) from labels known by hand: numbered by ascending label, the statistics over each label's distinct positions"""
    pos, label = np.asarray(pos, np.int64).reshape(-1, 3), np.asarray(label, np.uint32).reshape(-1)
    firsts = np.unique(label)
    ids = np.searchsorted(firsts, label).astype(np.uint32)
    table = np.zeros(len(firsts), P.PIECE)
    order = np.argsort(ids, kind="stable")
    cuts = np.searchsorted(ids[order], np.arange(len(firsts) + 1))
    for c in range(len(firsts)):
        mine = np.unique(pos[order[cuts[c]:cuts[c + 1]]], axis=0)
        table[c]["first"], table[c]["voxels"] = firsts[c], len(mine)
        table[c]["min"], table[c]["max"], table[c]["sum"] = mine.min(axis=0), mine.max(axis=0), mine.sum(axis=0)
    return label, ids, table


def same_want(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2].tobytes() == b[2].tobytes()


# ---- the rule at its edges ---------------------------------------------------------------------------------------------------------
def test_lists_of_none_one_and_two(ctx):
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.zeros(0, P.PIECE))
    check(ctx, np.zeros((0, 3), np.int16), {c: empty for c in K.CONNECTIVITIES}, "n = 0")
    for pos in ([[7, -9, 11]], [[7, -9, 11], [7, -9, 11]], [[7, -9, 11], [-7, 9, -11]]):
        check(ctx, pos, modelled(pos), f"n = {len(pos)}")
    # the wrapper: tensors of the documented types, a numpy list uploaded first
    label, ids, table = ctx.component_table(np.array([[0, 0, 0], [5, 5, 5], [0, 1, 0], [5, 5, 5]], np.int16))
    assert all(t.device == DEV for t in (label, ids, *table.values()))
    assert (label.dtype, ids.dtype) == (torch.uint32, torch.uint32) and sorted(table) == sorted(P.FIELDS)
    assert [table[f].dtype for f in P.FIELDS] == [torch.uint32, torch.uint32, torch.int16, torch.int16, torch.int64]
    assert (label.cpu().numpy().tolist(), ids.cpu().numpy().tolist()) == ([0, 1, 0, 1], [0, 1, 0, 1])
    assert (table["first"].cpu().numpy().tolist(), table["voxels"].cpu().numpy().tolist()) == ([0, 1], [2, 1])
    assert table["min"].cpu().numpy().tolist() == [[0, 0, 0], [5, 5, 5]] and table["max"].cpu().numpy().tolist() == [[0, 1, 0], [5, 5, 5]]
    assert table["sum"].cpu().numpy().tolist() == [[0, 1, 0], [5, 5, 5]]
    label, ids, table = ctx.component_table(torch.zeros((0, 3), dtype=torch.int16, device=DEV), 26)
    assert tuple(label.shape) == tuple(ids.shape) == (0,) and tuple(table["min"].shape) == (0, 3) and tuple(table["sum"].shape) == (0, 3)


PAIRS = {"face": ((3, 4, 5), (3, 5, 5), [1, 1, 1]), "edge": ((3, 4, 5), (4, 5, 5), [2, 1, 1]), "corner": ((3, 4, 5), (4, 3, 6), [2, 2, 1]),
         "wrap": ((32767, 0, 0), (-32768, 0, 0), [2, 2, 2]), "wrap on every axis": ((32767, 32767, 32767), (-32768, -32768, -32768), [2, 2, 2])}


@pytest.mark.parametrize("name", list(PAIRS))
def test_adjacency_pairs(ctx, name):
    a, b, counts = PAIRS[name]
    for pair in ([a, b], [b, a]):
        want = modelled(pair)
        assert [len(want[c][2]) for c in K.CONNECTIVITIES] == counts
        if "wrap" in name:
            assert all(np.array_equal(want[c][2]["min"], want[c][2]["max"]) for c in K.CONNECTIVITIES)
        check(ctx, pair, want, name)


def test_each_output_is_optional(ctx):
    rng = np.random.default_rng(11)
    cells = np.unique(rng.integers(-6, 7, (600, 3)), axis=0)
    cells = cells[rng.permutation(len(cells))[:300]]
    pos = np.repeat(cells, rng.integers(1, 5, 300), axis=0)      # listed one to four times
    pos = pos[rng.permutation(len(pos))].astype(np.int16)
    want = modelled(pos)
    assert 1 < len(want[6][2]) < 300 and int(want[6][2]["voxels"].sum()) == 300 < len(pos)      # distinct positions, not entries
    check(ctx, pos, want, "duplicates")
    n, d_pos = len(pos), on_device(pos)
    w_label, w_ids, w_table = want[18]
    k = len(w_table)
    for use in itertools.product((False, True), repeat=3):
        label, ids, info = Words(n), Words(n), Words(k * PIECE_WORDS)
        given = [b.ptr if u else None for b, u in zip((label, ids, info), use)]
        assert raw_table(ctx, d_pos, n, 18, *given, k) == (0, k), use
        for buf, u, expect in zip((label, ids), use, (w_label, w_ids)):
            assert buf.guards_hold() and (np.array_equal(buf.words(), expect) if u else buf.untouched()), use
        assert info.guards_hold() and (info.pieces(k).tobytes() == w_table.tobytes() if use[2] else info.untouched()), use


# ---- runs that end at a wave's and a block's edge -------------------------------------------------------------------------------------
RUNS = (255, 256, 257, 2047, 2048, 2049, 4097)


@functools.lru_cache(maxsize=None)
def run_list():
    """separated runs along x of RUNS voxels, in path order: (pos, label by hand)"""
    pos, label, x = [], [], -6000
    for run in RUNS:
        label += [len(pos)] * run
        pos += [(x + i, 5, -5) for i in range(run)]
        x += run + 1                                  # one empty cell between two runs
    pos = np.array(pos, np.int64)
    assert (np.diff(K.path_keys(pos)) > 0).all()
    return pos, np.array(label, np.uint32)


@pytest.mark.parametrize("order", ["path order", "shuffled"])
def test_separated_runs_along_x(ctx, order):
    pos, label = run_list()
    if order == "shuffled":
        perm = np.random.default_rng(7).permutation(len(pos))
        pos = pos[perm]
        first = {}
        for i, r in enumerate(label[perm].tolist()):
            first.setdefault(r, i)
        label = np.array([first[r] for r in label[perm].tolist()], np.uint32)
    hand = hand_table(pos, label)
    assert sorted(hand[2]["voxels"].tolist()) == sorted(RUNS)
    if order == "shuffled":
        assert hand[2]["voxels"].tolist() != list(RUNS)      # numbered by label, which is no longer key order
    model = P.component_table(pos, 6)
    assert same_want(hand, model)
    check(ctx, pos, {c: hand for c in K.CONNECTIVITIES}, f"runs, {order}")


# ---- runs of length 1 ----------------------------------------------------------------------------------------------------------------
def test_two_interleaved_combs(ctx):
    a, b, bridge = combs()
    for what, pos in (("joined", np.concatenate([a, b, bridge])), ("not joined", np.concatenate([b, a]))):
        want = modelled(pos)
        assert [len(want[c][2]) for c in K.CONNECTIVITIES] == ([1, 1, 1] if what == "joined" else [2, 2, 2])
        check(ctx, pos, want, f"combs {what}")
        shuffled = pos[np.random.default_rng(1).permutation(len(pos))]
        check(ctx, shuffled, modelled(shuffled), f"combs {what}, shuffled")


def test_checkerboard(ctx):
    board = np.argwhere(np.indices((16, 16, 16)).sum(axis=0) % 2 == 0) - 8
    want = modelled(board)
    assert [len(want[c][2]) for c in K.CONNECTIVITIES] == [2048, 1, 1]
    check(ctx, board, want, "checkerboard")
    shuffled = board[np.random.default_rng(3).permutation(2048)]
    check(ctx, shuffled, modelled(shuffled), "checkerboard, shuffled")


# ---- one component over many blocks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["head first", "tail first", "shuffled"])
def test_the_chain_through_32_cubed(ctx, order):
    small = chain(16)
    assert same_want(hand_table(small, np.zeros(len(small), np.uint32)), P.component_table(small, 6))      # hand_table on a chain
    pos = chain(32)
    assert len(pos) == 65535
    pos = {"head first": pos, "tail first": pos[::-1], "shuffled": pos[np.random.default_rng(32).permutation(len(pos))]}[order]
    hand = hand_table(pos, np.zeros(len(pos), np.uint32))      # one component at every connectivity (test_gpu_components.py)
    assert len(hand[2]) == 1 and hand[2]["voxels"][0] == 65535
    check(ctx, pos, {c: hand for c in K.CONNECTIVITIES}, f"chain {order}")


def test_sums_beyond_32_bits(ctx):
    """two solid blocks of 64 x 64 x 40 at the two ends of the int16 range: each coordinate sum exceeds 2^32 in magnitude"""
    block = np.stack(np.meshgrid(np.arange(64), np.arange(64), np.arange(40), indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int64)
    high = block + (32768 - 64, 32768 - 64, 32768 - 40)
    low = -1 - high                                           # the mirror: its least corner is (-32768, -32768, -32768)
    assert high.max(axis=0).tolist() == [32767] * 3 and low.min(axis=0).tolist() == [-32768] * 3 and len(high) == 163840
    pos = np.concatenate([high, low])
    hand = hand_table(pos, np.repeat(np.array([0, len(high)], np.uint32), len(high)))
    assert hand[2]["voxels"].tolist() == [163840, 163840] and (np.abs(hand[2]["sum"]) > 1 << 32).all()
    assert (hand[2]["sum"][0] > 0).all() and (hand[2]["sum"][1] < 0).all()
    small = np.concatenate([high[:500], low[:500]])           # hand_table on the same shape, small enough for the model
    assert same_want(hand_table(small, np.repeat(np.array([0, 500], np.uint32), 500)), P.component_table(small, 26))
    check(ctx, pos, {c: hand for c in K.CONNECTIVITIES}, "two blocks")


# ---- the general case ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_tables(seed):
    cells, labels = random_list(seed)
    want = modelled(cells)
    assert all(np.array_equal(want[c][0], labels[c][0]) for c in K.CONNECTIVITIES)
    return cells, want


def shifted(want, by):
    out = {}
    for conn, (label, ids, table) in want.items():
        moved = table.copy()
        moved["min"], moved["max"] = table["min"] + by, table["max"] + by
        moved["sum"] = table["sum"] + by * table["voxels"].astype(np.int64)[:, None]
        out[conn] = (label, ids, moved)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_grids(ctx, seed):
    cells, want = random_tables(seed)
    assert len(want[6][2]) > len(want[18][2]) > len(want[26][2]) >= 1
    check(ctx, cells - 20, shifted(want, -20), f"seed {seed}, around the origin")
    far = cells + (32768 - 40)
    assert far.max() == 32767
    if seed == 1:
        assert same_want(P.component_table(far, 18), shifted(want, 32768 - 40)[18])      # the shift of a table is exact
    check(ctx, far, shifted(want, 32768 - 40), f"seed {seed}, ending at 32767")


def test_a_list_at_an_odd_address(ctx):
    cells, _ = random_list(1)
    pos = np.ascontiguousarray(cells[:3001] - 20, np.int16)
    w_label, w_ids, w_table = P.component_table(pos, 18)
    n, k = len(pos), len(w_table)
    raw = torch.zeros(pos.nbytes + 8, dtype=torch.uint8, device=DEV)
    for off in (1, 2, 3):
        raw[off:off + pos.nbytes] = torch.as_tensor(pos.view(np.uint8).reshape(-1), device=DEV)
        torch.cuda.synchronize()
        label, ids, table, count = tabled(ctx, C.c_void_p(raw.data_ptr() + off), n, 18, k)
        assert count == k and np.array_equal(label, w_label) and np.array_equal(ids, w_ids), off
        assert_tables_equal(table, w_table, off)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx, H):
    n, k = 1025, 257
    pos = np.zeros((n, 3), np.int16)
    pos[:256, 0] = 2 * np.arange(256)                 # 256 voxels apart from each other
    pos[256:, 0], pos[256:, 1] = np.arange(n - 256), 5        # and one run
    assert len(P.component_table(pos, 26)[2]) == k
    d_pos = on_device(pos)
    label, ids, info = Words(n), Words(n), Words(k * PIECE_WORDS)

    def refused(*args, count=0xDEAD):
        assert raw_table(ctx, *args) == (H.E_INVALID, count), args
        assert last_error(ctx)
        assert label.untouched() and ids.untouched() and info.untouched()

    for connectivity in (0, 7, 27):
        refused(d_pos, n, connectivity, label.ptr, ids.ptr, info.ptr, k)
        refused(d_pos, n, connectivity, None, None, None, 0)
    host = [np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(k, P.PIECE)]
    refused(C.c_void_p(pos.ctypes.data), n, 6, label.ptr, ids.ptr, info.ptr, k)      # host memory, pageable
    refused(torch.as_tensor(pos).pin_memory(), n, 6, label.ptr, ids.ptr, info.ptr, k)      # ... and pinned
    refused(None, n, 6, label.ptr, ids.ptr, info.ptr, k)
    refused(d_pos, n, 6, C.c_void_p(host[0].ctypes.data), ids.ptr, info.ptr, k)
    refused(d_pos, n, 6, label.ptr, C.c_void_p(host[1].ctypes.data), info.ptr, k)
    refused(d_pos, n, 6, label.ptr, ids.ptr, C.c_void_p(host[2].ctypes.data), k)
    assert not any(a.view(np.uint8).any() for a in host)
    refused(d_pos, n, 6, C.c_void_p(label.ptr.value + 2), ids.ptr, info.ptr, k)      # misaligned by 2 bytes
    refused(d_pos, n, 6, label.ptr, C.c_void_p(ids.ptr.value + 2), info.ptr, k)
    refused(d_pos, n, 6, label.ptr, ids.ptr, C.c_void_p(info.ptr.value + 4), k)      # ... and info by 4
    refused(d_pos, 1 << 32, 6, label.ptr, ids.ptr, info.ptr, k)                      # checked before any pointer is looked at
    refused(None, 1 << 32, 6, None, None, None, 0)
    refused(d_pos, n, 6, label.ptr, ids.ptr, info.ptr, k - 1, count=k)               # room for one record less: the count all the same
    assert last_error(ctx) == f"vxrt_component_table_device: {k} components, room for {k - 1}"     # the entry point that was called
    refused(d_pos, n, 6, None, None, info.ptr, 0, count=k)
    # arrays one entry short.  Each is an allocation of its own, because what the library can see is the allocation: a torch tensor
    # lies in a larger block of torch's allocator.  1024 words and 256 records are whole pages, so no rounding hides the missing entry
    hip = C.CDLL("libamdhip64.so")
    short, small = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (n - 1))) == 0
    assert hip.hipMalloc(C.byref(small), C.c_size_t(P.PIECE.itemsize * (k - 1))) == 0 and P.PIECE.itemsize * (k - 1) % 4096 == 0
    refused(d_pos, n, 6, short, ids.ptr, info.ptr, k)
    assert "label" in last_error(ctx)
    refused(d_pos, n, 6, label.ptr, short, info.ptr, k)
    assert "id" in last_error(ctx)
    refused(d_pos, n, 6, label.ptr, ids.ptr, small, k)
    assert "info" in last_error(ctx)
    rest = C.c_void_p(d_pos.data_ptr() + 6)                                              # the list without its first voxel
    assert raw_table(ctx, rest, n - 1, 6, short, None, small, k - 1) == (0, k - 1)       # they hold n - 1 entries and k - 1 records
    assert hip.hipFree(short) == 0 and hip.hipFree(small) == 0
    assert ctx._L.vxrt_component_table_device(ctx._h, ptr(d_pos), C.c_size_t(n), C.c_uint32(6), label.ptr, ids.ptr, info.ptr, C.c_size_t(k),
                                              None) == H.E_INVALID
    assert label.untouched() and ids.untouched() and info.untouched()
    # ... and the valid call is accepted afterwards
    assert raw_table(ctx, d_pos, n, 6, label.ptr, ids.ptr, info.ptr, k) == (0, k)
    want = P.component_table(pos, 6)
    assert np.array_equal(label.words(), want[0]) and np.array_equal(ids.words(), want[1]) and info.pieces(k).tobytes() == want[2].tobytes()


# ---- the scene call ------------------------------------------------------------------------------------------------------------------
def voxel_dict(pos, mrgb):
    return {tuple(p): tuple(b) for p, b in zip(np.asarray(pos).tolist(), np.asarray(mrgb).tolist())}


@pytest.fixture(scope="module")
def sponge(H):
    """the level-3 sponge as get_voxels gives it: (pos, mrgb, dict, anchor box = its lowest y layer, its least corner)"""
    with make_ctx(H, CFG) as c:
        c.set_menger(3, 0, MENGER_MRGB)
        pos, mrgb = c.get_voxels()
    assert len(pos) == 8000
    lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
    anchor = (tuple(lo.tolist()), (int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))
    return pos, mrgb, voxel_dict(pos, mrgb), anchor, lo


def cut_sponge(c, sponge, gone):
    """a context's sponge with the voxels where gone(x, y, z), relative to the least corner, cleared -> the model's dict"""
    pos, mrgb, voxels, anchor, lo = sponge
    mask = np.array([bool(gone(*(p - lo))) for p in pos.astype(int)])
    c.set_menger(3, 0, MENGER_MRGB)
    if mask.any():
        c.clear_voxels_device(on_device(pos[mask]))
    return {tuple(p): voxels[tuple(p)] for p in pos[~mask].tolist()}


def several_cuts(x, y, z):
    """two layers, two planes through the top slab and a column of the middle one: nine pieces, the least of 21 voxels"""
    return y in (8, 17) or (y > 17 and (x == 24 or z == 24)) or (8 < y < 17 and x == 2 and z < 9)


def assert_pieces(c, anchor, conn, sizes, want, what, H):
    """count-only, a guarded call with exactly enough room, and the wrapper, against want = the model's (pos, mrgb, piece, table)"""
    w_pos, w_mrgb, w_piece, w_table = want
    n, k = len(w_pos), len(w_table)
    assert raw_pieces(c, *anchor, conn, *sizes, None, None, None, 0, None, 0) == (0, n, k), f"{what}: count only"
    gp, gm = guarded(n + 2)
    piece, info = Words(n + 2), Words((k + 1) * PIECE_WORDS)
    assert raw_pieces(c, *anchor, conn, *sizes, gp, gm, piece.ptr, n, info.ptr, k) == (0, n, k), (what, last_error(c))
    assert np.array_equal(gp[:n].cpu().numpy(), w_pos) and np.array_equal(gm[:n].cpu().numpy(), w_mrgb), f"{what}: positions and bytes"
    assert untouched(gp[n:], gm[n:]) and piece.guards_hold(n) and info.guards_hold(k * PIECE_WORDS), f"{what}: guards"
    assert np.array_equal(piece.words(n), w_piece), f"{what}: piece"
    assert_tables_equal(info.pieces(k), w_table, what)
    pos, mrgb, pc, table = c.detached_pieces(*anchor, connectivity=conn, min_voxels=sizes[0], max_voxels=None if sizes[1] == EVERY else sizes[1])
    assert pos.dtype == torch.int16 and mrgb.dtype == torch.uint8 and pc.dtype == torch.uint32 and pos.device == DEV, what
    assert tuple(pos.shape) == (n, 3) and tuple(mrgb.shape) == (n, 4) and tuple(pc.shape) == (n,), what
    assert np.array_equal(pos.cpu().numpy(), w_pos) and np.array_equal(mrgb.cpu().numpy(), w_mrgb) and np.array_equal(pc.cpu().numpy(), w_piece), what
    for f in P.FIELDS:
        assert np.array_equal(table[f].cpu().numpy(), w_table[f]), (what, f)
    return pos, mrgb, pc, table


@pytest.mark.parametrize("conn", [6, 26])
def test_an_untouched_scene_and_one_layer_cleared(H, sponge, conn):
    pos, mrgb, voxels, anchor, lo = sponge
    with make_ctx(H, CFG) as c:
        model = cut_sponge(c, sponge, lambda x, y, z: False)
        none = (pos[:0], mrgb[:0], np.zeros(0, np.uint32), np.zeros(0, P.PIECE))
        assert_pieces(c, anchor, conn, (0, EVERY), none, "untouched", H)
        # an empty anchor box, or one that misses the scene: every component, and the sponge is one
        whole = P.detached_pieces(model, (0, 0, 0), (0, 5, 5), conn)
        assert np.array_equal(whole[0], pos) and np.array_equal(whole[1], mrgb) and whole[3]["voxels"].tolist() == [8000]
        assert_pieces(c, ((0, 0, 0), (0, 5, 5)), conn, (0, EVERY), whole, "an empty anchor box", H)
        got = assert_pieces(c, ((100, 100, 100), (200, 200, 200)), conn, (0, EVERY), whole, "an anchor box that misses the scene", H)
        everything = c.get_voxels_device()
        assert torch.equal(got[0], everything[0]) and torch.equal(got[1], everything[1])
        # one whole layer cleared: everything above it is one piece
        model = cut_sponge(c, sponge, lambda x, y, z: y == 8)
        want = P.detached_pieces(model, *anchor, conn)
        assert len(want[0]) == 4800 and want[3]["voxels"].tolist() == [4800] and not want[2].any()
        records = c.read_scene()
        got = assert_pieces(c, anchor, conn, (0, EVERY), want, "a layer cleared", H)
        mere = c.detached_voxels(*anchor, connectivity=conn)
        assert torch.equal(got[0], mere[0]) and torch.equal(got[1], mere[1])
        assert np.array_equal(mere[0].cpu().numpy(), want[0]) and np.array_equal(mere[1].cpu().numpy(), want[1]), "detached_voxels against the model"
        for a, b in zip(c.read_scene(), records):
            assert np.array_equal(a, b), "the call changed the scene"


@pytest.mark.parametrize("conn", [6, 26])
def test_pieces_of_different_sizes_and_the_size_filter(H, sponge, conn):
    pos, mrgb, voxels, anchor, lo = sponge
    with make_ctx(H, CFG) as c:
        model = cut_sponge(c, sponge, several_cuts)
        full = P.detached_pieces(model, *anchor, conn)
        sizes = full[3]["voxels"].tolist()
        least, most = min(sizes), max(sizes)
        assert len(sizes) >= 3 and len(set(sizes)) >= 3 and sizes.count(least) == 1 and sizes.count(most) == 1 and most > 20 * least
        gap = next(v for v in range(least + 1, most) if v not in sizes)
        records = c.read_scene()
        ranges = {"the full range": (0, EVERY), "only the smallest": (0, least), "only the largest": (most, EVERY), "none": (gap, gap),
                  "min > max": (most, least), "a middle range": (least + 1, most - 1)}
        for name, rng in ranges.items():
            want = P.detached_pieces(model, *anchor, conn, *rng)
            k = {"the full range": len(sizes), "only the smallest": 1, "only the largest": 1, "none": 0, "min > max": 0, "a middle range": len(sizes) - 2}[name]
            assert len(want[3]) == k, name
            got = assert_pieces(c, anchor, conn, rng, want, name, H)
            if len(want[0]):
                # the first identity: the table of the returned list is the returned piece and table
                label, ids, table = c.component_table(got[0], conn)
                assert np.array_equal(host(ids), host(got[2])) and all(np.array_equal(host(table[f]), host(got[3][f])) for f in P.FIELDS), name
                assert np.array_equal(host(label), host(got[3]["first"])[host(got[2])]), name
        # the second identity: the full range is detached_voxels
        mere = c.detached_voxels(*anchor, connectivity=conn)
        assert np.array_equal(mere[0].cpu().numpy(), full[0]) and np.array_equal(mere[1].cpu().numpy(), full[1])
        for a, b in zip(c.read_scene(), records):
            assert np.array_equal(a, b), "the calls changed the scene"
        # room for one voxel less, or for one piece less: the counts, an error and nothing written
        n, k = len(full[0]), len(sizes)
        gp, gm = guarded(n + 2)
        piece, info = Words(n), Words(k * PIECE_WORDS)
        for cap, info_cap in ((n - 1, k), (n, k - 1), (0, 0)):
            assert raw_pieces(c, *anchor, conn, 0, EVERY, gp, gm, piece.ptr, cap, info.ptr, info_cap) == (H.E_INVALID, n, k)
            assert last_error(c).startswith("vxrt_detached_pieces_device: ") and "room for" in last_error(c)     # the entry point that was called
            assert untouched(gp, gm) and piece.untouched() and info.untouched()
        assert raw_pieces(c, *anchor, conn, 0, EVERY, None, None, piece.ptr, n - 1, None, 0) == (H.E_INVALID, n, k) and piece.untouched()
        # refusals: one of pos and mrgb, a null anchor, the connectivity, misaligned piece and info
        assert raw_pieces(c, *anchor, conn, 0, EVERY, gp, None, piece.ptr, n, info.ptr, k)[0] == H.E_INVALID
        assert raw_pieces(c, None, anchor[1], conn, 0, EVERY, gp, gm, piece.ptr, n, info.ptr, k)[0] == H.E_INVALID
        for bad in (0, 7, 27):
            assert raw_pieces(c, *anchor, bad, 0, EVERY, gp, gm, piece.ptr, n, info.ptr, k) == (H.E_INVALID, 0xDEAD, 0xBEEF)
        assert raw_pieces(c, *anchor, conn, 0, EVERY, gp, gm, C.c_void_p(piece.ptr.value + 2), n, info.ptr, k) == (H.E_INVALID, 0xDEAD, 0xBEEF)
        assert raw_pieces(c, *anchor, conn, 0, EVERY, gp, gm, piece.ptr, n, C.c_void_p(info.ptr.value + 4), k) == (H.E_INVALID, 0xDEAD, 0xBEEF)
        assert untouched(gp, gm) and piece.untouched() and info.untouched()
        # each output alone
        assert raw_pieces(c, *anchor, conn, 0, EVERY, None, None, piece.ptr, n, None, 0) == (0, n, k) and np.array_equal(piece.words(), full[2])
        assert raw_pieces(c, *anchor, conn, 0, EVERY, None, None, None, 0, info.ptr, k) == (0, n, k) and info.pieces(k).tobytes() == full[3].tobytes()
        assert untouched(gp, gm) and piece.guards_hold() and info.guards_hold()
        # odd output addresses for pos and mrgb
        bp = torch.full((6 * n + 8,), GUARD_MRGB, dtype=torch.uint8, device=DEV)
        bm = torch.full((4 * n + 8,), GUARD_MRGB, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        assert raw_pieces(c, *anchor, conn, 0, EVERY, C.c_void_p(bp.data_ptr() + 1), C.c_void_p(bm.data_ptr() + 2), piece.ptr, n, info.ptr, k) == (0, n, k)
        assert bp[1:1 + 6 * n].cpu().numpy().tobytes() == full[0].tobytes() and bm[2:2 + 4 * n].cpu().numpy().tobytes() == full[1].tobytes()
        assert bool((bp[:1] == GUARD_MRGB).all()) and bool((bp[1 + 6 * n:] == GUARD_MRGB).all())
        assert bool((bm[:2] == GUARD_MRGB).all()) and bool((bm[2 + 4 * n:] == GUARD_MRGB).all())
        # the same scene in treelet order, which the extract reads and the editor refuses
        with make_ctx(H, (1, 1, 1, 1), tuning=[(H.OPT_NODE_ORDER, 2)]) as t:
            t.recreate_octree(np.array(list(model), np.int16), np.array(list(model.values()), np.uint8))
            assert t.stats().node_order == 2
            assert_pieces(t, anchor, conn, (0, EVERY), full, "treelet order", H)
            assert_pieces(t, anchor, conn, (0, least), P.detached_pieces(model, *anchor, conn, 0, least), "treelet order, the smallest", H)


def host(t):
    return t.cpu().numpy()


def staircase(voxels, y):
    """test_gpu_components.py: (x, z) with the sponge solid at (x, y - 1, z), (x, y, z), (x + 1, y + 1, z + 1), (x + 1, y + 2, z + 1)"""
    for x, yy, z in sorted(voxels):
        if yy == y and all(c in voxels for c in ((x, y - 1, z), (x + 1, y + 1, z + 1), (x + 1, y + 2, z + 1))):
            return x, z
    raise AssertionError("no staircase")


def test_a_staircase_holds_by_its_corners_only(H, sponge):
    pos, mrgb, voxels, anchor, lo = sponge
    layer = int(lo[1]) + 8
    x, z = staircase(voxels, layer)
    keep = {(x, layer, z), (x + 1, layer + 1, z + 1)}
    above = int((pos[:, 1] > layer + 1).sum())
    with make_ctx(H, CFG) as c:
        model = cut_sponge(c, sponge, lambda a, b, d: b in (8, 9) and (a + lo[0], b + lo[1], d + lo[2]) not in keep)
        assert len(model) == 8000 - int(np.isin(pos[:, 1], (layer, layer + 1)).sum()) + 2
        for conn in K.CONNECTIVITIES:
            want = P.detached_pieces(model, *anchor, conn)
            assert want[3]["voxels"].tolist() == ([above + 1] if conn != 26 else [])      # the upper step falls with the upper half
            assert_pieces(c, anchor, conn, (0, EVERY), want, f"staircase, {conn}", H)


@pytest.mark.parametrize("conn", [6, 26])
def test_drop_detached_pieces_up_to_a_size(H, sponge, conn):
    pos, mrgb, voxels, anchor, lo = sponge
    with make_ctx(H, CFG) as c, make_ctx(H, CFG) as twin:
        model = cut_sponge(c, sponge, several_cuts)
        cut_sponge(twin, sponge, several_cuts)
        limit = 300
        want = P.detached_pieces(model, *anchor, conn, 0, limit)
        kept = P.detached_pieces(model, *anchor, conn, limit + 1, EVERY)
        assert len(want[3]) >= 2 and len(kept[3]) >= 2
        twin.clear_voxels_device(on_device(want[0]))
        removed = c.drop_detached_pieces(*anchor, connectivity=conn, max_voxels=limit)
        assert np.array_equal(removed[0].cpu().numpy(), want[0]) and np.array_equal(removed[1].cpu().numpy(), want[1])
        assert np.array_equal(removed[2].cpu().numpy(), want[2]) and all(np.array_equal(removed[3][f].cpu().numpy(), want[3][f]) for f in P.FIELDS)
        assert_same_scene(c, twin, "drop_detached_pieces against clearing the model's list")
        dropped = set(map(tuple, want[0].tolist()))
        left = {p: b for p, b in model.items() if p not in dropped}
        assert c.count_voxels() == len(left) == len(model) - len(want[0])
        # the pieces above the limit are still in the scene and still detached
        assert_pieces(c, anchor, conn, (0, EVERY), kept, "what stayed", H)
        after = P.detached_pieces(left, *anchor, conn)
        assert np.array_equal(after[0], kept[0]) and np.array_equal(after[2], kept[2]) and after[3].tobytes() == kept[3].tobytes()
        assert tuple(c.drop_detached_pieces(*anchor, connectivity=conn, max_voxels=limit)[0].shape) == (0, 3)      # nothing that small is left
        c.fit_scene_depth()
        c.compact_scene()
        with make_ctx(H, CFG) as ref:
            ref.recreate_octree(np.array(sorted(left), np.int16), np.array([left[p] for p in sorted(left)], np.uint8))
            assert ref.scene_depth == c.scene_depth
            assert_same_scene(c, ref, "drop_detached_pieces, fitted and compacted, against a fresh build of the remainder")


def test_no_scene_and_an_empty_scene(ctx, H):
    with pytest.raises(H.VxrtError) as e:
        ctx.detached_pieces((0, 0, 0), (1, 1, 1))
    assert e.value.status == H.E_NOSCENE
    assert raw_pieces(ctx, (0, 0, 0), (1, 1, 1), 6, 0, EVERY, None, None, None, 0, None, 0) == (H.E_NOSCENE, 0xDEAD, 0xBEEF)
    with make_ctx(H, CFG) as c:
        c.recreate_octree(np.array([[1, 2, 3]], np.int16), np.array([[1, 2, 3, 4]], np.uint8))
        c.clear_voxels(np.array([[1, 2, 3]], np.int16))
        assert raw_pieces(c, (0, 0, 0), (1, 1, 1), 6, 0, EVERY, None, None, None, 0, None, 0) == (0, 0, 0)
        pos, mrgb, piece, table = c.detached_pieces((0, 0, 0), (1, 1, 1))
        assert tuple(pos.shape) == (0, 3) and tuple(mrgb.shape) == (0, 4) and tuple(piece.shape) == (0,) and tuple(table["sum"].shape) == (0, 3)
        assert tuple(c.drop_detached_pieces((0, 0, 0), (1, 1, 1))[0].shape) == (0, 3)
