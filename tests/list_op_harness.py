"""What the GPU tests of the operators on device voxel lists share (test_gpu_transform.py, test_gpu_setops.py, test_gpu_morph.py):
device memory between guard bytes, and check_call, the ladder every case of theirs goes through against its model."""
import ctypes as C

import numpy as np
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import transform_model as T

DEV = torch.device("cuda", 0)
GUARD = 0xA5
GUARD_BYTES = 64


def on_device(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def last_error(ctx):
    return (ctx._L.vxrt_last_error() or b"").decode()


class Bytes:
    """n bytes of device memory between guard bytes, starting `shift` bytes past a 16-byte boundary"""
    def __init__(self, n, shift=0, fill=None):
        self.n, self.lead = n, GUARD_BYTES + shift
        self.buf = torch.full((n + 2 * GUARD_BYTES + 16,), GUARD, dtype=torch.uint8, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        if fill is not None and n:
            self.buf[self.lead:self.lead + n] = on_device(np.ascontiguousarray(fill).view(np.uint8).reshape(-1))
        torch.cuda.synchronize()
        self.ptr = C.c_void_p(self.buf.data_ptr() + self.lead)

    def all(self):
        return self.buf.cpu().numpy()

    def guards_hold(self):
        b = self.all()
        return bool((b[:self.lead] == GUARD).all()) and bool((b[self.lead + self.n:] == GUARD).all())

    def untouched(self):
        return bool((self.all() == GUARD).all())

    def data(self):
        return self.all()[self.lead:self.lead + self.n].copy()


def colours(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 4)).astype(np.uint8)


def by_path(pos):
    """Distinct positions, in path order."""
    return np.array(sorted({tuple(p) for p in np.asarray(pos).tolist()}, key=T.path_key), np.int16).reshape(-1, 3)


def check_call(ctx, raw, wrapper, inputs, want_pos, want_mrgb, what, shift=0):
    """One set of arguments through every form of an operator's call against the model's (want_pos, want_mrgb) -> (pos, mrgb) of
    the result.  inputs: (name, array or None) per device array the call reads, in its order, int16 [n,3] or uint8 [n,4], the first
    list's positions and bytes first: the result has bytes where that list has.  raw(ptr, out_pos, out_mrgb, cap): the C call over
    the inputs' addresses -> (status, *n_out); wrapper(dev, cap): the Context method over the inputs as device tensors."""
    with_vals = inputs[1][1] is not None
    k = len(want_pos)
    ins = [None if v is None else Bytes(v.nbytes, shift, v) for _, v in inputs]
    ptr = [None if b is None else b.ptr for b in ins]
    assert raw(ptr, None, None, 0) == (0, k), (what, "count only", last_error(ctx))
    assert raw(ptr, None, None, 12345) == (0, k), (what, "count only ignores cap")
    outs = []
    for turn in range(2):
        out_pos, out_mrgb = Bytes(6 * k, shift), (Bytes(4 * k, shift) if with_vals else None)
        assert raw(ptr, out_pos.ptr, None if out_mrgb is None else out_mrgb.ptr, k) == (0, k), (what, f"call {turn}", last_error(ctx))
        assert out_pos.guards_hold() and (out_mrgb is None or out_mrgb.guards_hold()), f"{what}: guard bytes"
        outs.append((out_pos, out_mrgb))
    got_pos = outs[0][0].data().view(np.int16).reshape(-1, 3)
    assert np.array_equal(got_pos, want_pos), f"{what}: {int((got_pos != want_pos).any(axis=1).sum())} of {k} positions differ"
    got_mrgb = None
    if with_vals:
        got_mrgb = outs[0][1].data().reshape(-1, 4)
        assert np.array_equal(got_mrgb, want_mrgb), f"{what}: {int((got_mrgb != want_mrgb).any(axis=1).sum())} of {k} voxels' bytes differ"
    assert outs[1][0].all().tobytes() == outs[0][0].all().tobytes(), f"{what}: a second call"
    assert not with_vals or outs[1][1].all().tobytes() == outs[0][1].all().tobytes(), f"{what}: a second call"
    for b, (name, v) in zip(ins, inputs):
        assert b is None or (b.guards_hold() and b.data().tobytes() == v.tobytes()), f"{what}: {name} was written"
    # the wrapper, counting first and with room to spare
    dev = [None if v is None else on_device(v) for _, v in inputs]
    for cap in (None, k + 3):
        w_pos, w_mrgb = wrapper(dev, cap)
        assert w_pos.dtype == torch.int16 and w_pos.device == DEV and tuple(w_pos.shape) == (k, 3), what
        assert np.array_equal(w_pos.cpu().numpy(), want_pos), f"{what}: the wrapper"
        assert (w_mrgb is None) == (not with_vals)
        if with_vals:
            assert w_mrgb.dtype == torch.uint8 and tuple(w_mrgb.shape) == (k, 4) and np.array_equal(w_mrgb.cpu().numpy(), want_mrgb), f"{what}: the wrapper"
    return got_pos, got_mrgb
