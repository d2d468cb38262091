"""GPU: the run heads of sorted keys (csrc/run_heads.h) through vxrt_debug_run_heads (include/vxrt_debug.h), against numpy.

For sorted keys the heads are the first entry of each run of keys >> shift; the call gives each head's shifted key and, with words,
that entry's word.  The sizes are chosen for the kernel's geometry (2048 entries a block, 8 a thread, side by side), the runs so that
heads fall on the first and on the last entry of a block and of a thread.  Every case goes through the counting call, the emitting
call between guard bytes, and a call with room for one head less, which is refused and writes nothing."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

from list_op_harness import Bytes, last_error

pytestmark = pytest.mark.gpu

SPAN, ITEMS = 2048, 8
SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097)


@pytest.fixture(scope="module")
def ctx(H):
    with H.Context(32, 32) as c:      # no scene is loaded: the call needs none
        yield c


def raw(ctx, keys, words, n, shift, out_keys, out_words, cap):
    """The C call over raw addresses -> (status, *n_out)."""
    torch.cuda.synchronize()
    got = C.c_size_t(0xDEAD)
    rc = ctx._L.vxrt_debug_run_heads(ctx._h, keys, words, C.c_size_t(n), C.c_uint32(shift), out_keys, out_words, C.c_size_t(cap), C.byref(got))
    return rc, got.value


def expected(keys, words, shift):
    """The first entry of each run of keys >> shift -> (shifted keys, words or None), from the inputs alone."""
    cells = keys >> np.uint64(shift)
    heads = np.concatenate([[0], np.flatnonzero(cells[1:] != cells[:-1]) + 1]).astype(np.int64)
    return cells[heads], None if words is None else words[heads]


def check(H, ctx, keys, shift, what):
    """Sorted keys at a shift, without and with words, through every form of the call -> the number of heads."""
    keys = np.ascontiguousarray(keys, np.uint64)
    assert (keys[1:] >= keys[:-1]).all(), what
    n = len(keys)
    for words in (None, (np.arange(n, dtype=np.uint32) * np.uint32(2654435761) + np.uint32(17))):
        what_now = f"{what}, shift {shift}, {'with' if words is not None else 'without'} words"
        want_keys, want_words = expected(keys, words, shift)
        k = len(want_keys)
        d_keys = Bytes(keys.nbytes, 0, keys)
        d_words = None if words is None else Bytes(words.nbytes, 0, words)
        p_words = None if words is None else d_words.ptr
        assert raw(ctx, d_keys.ptr, p_words, n, shift, None, None, 0) == (0, k), (what_now, "count only", last_error(ctx))
        out_keys, out_words = Bytes(8 * k), (None if words is None else Bytes(4 * k))
        assert raw(ctx, d_keys.ptr, p_words, n, shift, out_keys.ptr, None if words is None else out_words.ptr, k) == (0, k), (what_now, last_error(ctx))
        assert out_keys.guards_hold() and (words is None or out_words.guards_hold()), f"{what_now}: guard bytes"
        got_keys = out_keys.data().view(np.uint64)
        assert np.array_equal(got_keys, want_keys), f"{what_now}: {int((got_keys != want_keys).sum())} of {k} keys differ"
        if words is not None:
            got_words = out_words.data().view(np.uint32)
            assert np.array_equal(got_words, want_words), f"{what_now}: {int((got_words != want_words).sum())} of {k} words differ"
        # room for one head less: refused, and nothing is written
        short_keys, short_words = Bytes(8 * k), (None if words is None else Bytes(4 * k))
        rc, _ = raw(ctx, d_keys.ptr, p_words, n, shift, short_keys.ptr, None if words is None else short_words.ptr, k - 1)
        assert rc == H.E_INVALID and f"{k} voxels, room for {k - 1}" in last_error(ctx), (what_now, rc, last_error(ctx))
        assert short_keys.untouched() and (words is None or short_words.untouched()), f"{what_now}: a refused call wrote"
        assert d_keys.guards_hold() and d_keys.data().tobytes() == keys.tobytes(), f"{what_now}: keys were written"
        assert words is None or (d_words.guards_hold() and d_words.data().tobytes() == words.tobytes()), f"{what_now}: words were written"
    return k


def runs_of(n, length, offset, shift, seed, top=0):
    """n sorted keys in runs of `length` entries above `shift`, the first run `offset` entries short, random bits below the shift."""
    run = (np.arange(n, dtype=np.uint64) + np.uint64(offset)) // np.uint64(length)
    low = np.random.default_rng(seed).integers(0, 1 << shift, n, dtype=np.uint64) if shift else np.zeros(n, np.uint64)
    return np.sort(np.uint64(top) | (run + np.uint64(3)) << np.uint64(shift) | low)


@pytest.mark.parametrize("n", SIZES)
def test_heads_at_block_and_thread_boundaries(H, ctx, n):
    for shift in (0, 5):
        assert check(H, ctx, runs_of(n, 1 << 40, 0, shift, 1), shift, f"{n} equal keys") == 1
        assert check(H, ctx, runs_of(n, 1, 0, shift, 2), shift, f"{n} distinct keys") == n
        # a head is the first entry of every block / thread; then its last entry, and the run goes on in the next
        for length in (SPAN, ITEMS):
            assert check(H, ctx, runs_of(n, length, 0, shift, 3), shift, f"{n} keys in runs of {length}") == (n + length - 1) // length
            assert check(H, ctx, runs_of(n, length, 1, shift, 4), shift, f"{n} keys in runs of {length}, one early") == (n + length) // length


@pytest.mark.parametrize("shift", (0, 5, 12))
def test_the_shift_decides(H, ctx, shift):
    n = 2 * SPAN + 1
    rng = np.random.default_rng(shift)
    below = np.sort(np.uint64(0x1234) << np.uint64(shift) | (rng.integers(0, 1 << shift, n, dtype=np.uint64) if shift else np.zeros(n, np.uint64)))
    assert check(H, ctx, below, shift, "keys that differ below the shift only") == 1
    above = np.where(np.arange(n) < SPAN + 1, np.uint64(0x40) << np.uint64(shift), np.uint64(0x41) << np.uint64(shift)).astype(np.uint64)
    assert check(H, ctx, above, shift, "keys that differ in the bit above the shift only") == 2
    assert check(H, ctx, runs_of(n, 5, 0, shift, 7, top=1 << 63), shift, "keys with bit 63 set") == (n + 4) // 5


def test_nothing_and_what_is_refused(H, ctx):
    # no keys: no launch, and no pointer is touched
    assert raw(ctx, C.c_void_p(8), C.c_void_p(4), 0, 0, C.c_void_p(16), C.c_void_p(12), 4) == (0, 0)
    assert raw(ctx, None, None, 0, 12, None, None, 0) == (0, 0)
    keys = Bytes(64, 0, np.arange(8, dtype=np.uint64))
    out = Bytes(64)
    got = C.c_size_t(0)
    L = ctx._L
    assert L.vxrt_debug_run_heads(None, keys.ptr, None, C.c_size_t(8), C.c_uint32(0), None, None, C.c_size_t(0), C.byref(got)) == H.E_INVALID
    assert L.vxrt_debug_run_heads(ctx._h, keys.ptr, None, C.c_size_t(8), C.c_uint32(0), None, None, C.c_size_t(0), None) == H.E_INVALID
    assert raw(ctx, keys.ptr, None, 8, 64, None, None, 0)[0] == H.E_INVALID and "shift" in last_error(ctx)
    assert raw(ctx, None, None, 8, 0, None, None, 0)[0] == H.E_INVALID and "null keys" in last_error(ctx)
    assert raw(ctx, keys.ptr, None, 8, 0, out.ptr, out.ptr, 8)[0] == H.E_INVALID and "out_words without words" in last_error(ctx)
    assert raw(ctx, keys.ptr, keys.ptr, 8, 0, None, out.ptr, 8)[0] == H.E_INVALID and "out_words without out_keys" in last_error(ctx)
    assert raw(ctx, C.c_void_p(keys.ptr.value + 4), None, 7, 0, None, None, 0)[0] == H.E_INVALID and "aligned" in last_error(ctx)
    assert out.untouched() and keys.guards_hold()
