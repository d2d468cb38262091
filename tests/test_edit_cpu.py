"""CPU: the edit extension's interface (include/vxrt_edit.h) — declared, exported with C linkage, refused without a device where it
must be — and the Python model of an edit batch that tests/test_gpu_edit.py checks the device against."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import edit_model as M
from conftest import ROOT


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vxrt_[a-z_0-9]+)\s*\(", text)))


def test_edit_header_declares_both_entry_points():
    assert declared("vxrt_edit.h") == ["vxrt_edit_voxels", "vxrt_pick"]
    text = open(os.path.join(ROOT, "include", "vxrt_edit.h")).read()
    assert '#include "vxrt.h"' in text and "vxrt_pick_hit" in text
    assert "vxrt_edit.h" in open(os.path.join(ROOT, "include", "vxrt.h")).read()   # vxrt.h points at it


def test_contract_header_stays_within_40_entry_points():
    contract = declared("vxrt.h")
    assert len(contract) <= 40
    assert not set(contract) & set(declared("vxrt_edit.h"))


def test_library_exports_edit_symbols_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    for n in declared("vxrt_edit.h"):
        assert n in exported, n
    assert H.lib().vxrt_abi_version() == 6


def test_pick_hit_layout_matches_the_header(H):
    assert H.PICK_HIT_DTYPE.itemsize == 36
    assert [H.PICK_HIT_DTYPE.fields[n][1] for n in ("status", "time", "normal", "voxel", "leaf")] == [0, 4, 8, 20, 32]


def test_null_context_is_refused_without_a_device(H):
    L = H.lib()
    pos = np.zeros((1, 3), np.int16)
    mrgb = np.zeros((1, 4), np.uint8)
    assert L.vxrt_edit_voxels(None, pos.ctypes.data_as(C.c_void_p), mrgb.ctypes.data_as(C.c_void_p), C.c_size_t(1)) == -1
    assert L.vxrt_edit_voxels(None, None, None, C.c_size_t(0)) == -1
    o = np.zeros((1, 3), np.float32)
    out = np.zeros(1, H.PICK_HIT_DTYPE)
    assert L.vxrt_pick(None, o.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), C.c_size_t(1), out.ctypes.data_as(C.c_void_p)) == -1


def random_batches(seed, depth, base, count=6):
    """Seeded set / clear batches inside the root cube of `depth`, with duplicates inside batches and re-use across batches."""
    rng = np.random.default_rng(seed)
    lim = 1 << depth
    out = []
    known = np.array(sorted(base), np.int64).reshape(-1, 3)
    for k in range(count):
        n = int(rng.integers(1, 40))
        fresh = rng.integers(-lim, lim, size=(n, 3))
        old = known[rng.integers(0, len(known), size=n)] if len(known) else fresh
        pos = np.where(rng.random((n, 1)) < 0.5, fresh, old)
        pos = np.concatenate([pos, pos[: n // 3]])            # duplicates: the later entry wins
        mrgb = rng.integers(0, 256, size=(len(pos), 4))
        out.append((pos.astype(np.int16), None if k % 3 == 2 else mrgb.astype(np.uint8)))
    return out


def test_model_agrees_with_the_octree_builder(H):
    pos, mrgb = H.menger_voxels(2)
    words, depth = H.build_octree(pos, mrgb)
    model = M.from_list(pos, mrgb)
    assert M.decode_octree_words(words, depth) == model
    anchor = np.array([[-(1 << depth), -(1 << depth), -(1 << depth)], [(1 << depth) - 1] * 3], np.int16)
    M.apply(model, anchor, np.full((2, 4), 7, np.uint8))
    for bpos, bmrgb in random_batches(3, depth, model):
        M.apply(model, bpos, bmrgb)
        p, m = M.to_list(model)
        w, d = H.build_octree(p, m)
        assert d == depth
        assert M.decode_octree_words(w, d) == model
        svo, _, leaves, d2 = H.build_records(p, m)
        assert d2 == depth and M.decode_records(svo, leaves, d2) == model


def test_model_rules():
    model = {(0, 0, 0): 1}
    M.apply(model, [[1, 1, 1], [1, 1, 1]], [[1, 2, 3, 4], [0x85, 5, 6, 7]])
    assert model[(1, 1, 1)] == M.word([5, 5, 6, 7])                # last entry wins, material & 0x7f
    M.apply(model, [[2, 2, 2], [1, 1, 1]])                         # absent positions are ignored
    assert model == {(0, 0, 0): 1}
