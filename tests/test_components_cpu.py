"""CPU: the component labelling's interface (include/vxrt_components.h) — plain C, declared, exported with C linkage by both libraries,
refused without a context — the Python wrappers' argument checks, which run before any library call, and the model of the rule
(components_model.py) against something that does not follow its wording: a flood fill on a dense grid by repeated minimum over
shifted copies, and counts known by hand."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import components_model as K
from conftest import ROOT

FUNCTIONS = ["vxrt_detached_voxels_device", "vxrt_label_components_device"]
HEADER = "vxrt_components.h"
NEW_SOURCES = ("components.hip", "api_components.hip", "components.h")


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vxrt_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_exactly_the_two_entry_points():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt.h"' in text
    assert "do not wrap" in text and "least index" in text
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", hdr], capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'int main(void) {\n'
                   '    size_t n = 0;\n'
                   '    const int32_t lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};\n'
                   '    int a = vxrt_label_components_device(0, 0, 0, 6, 0, &n);\n'
                   '    int b = vxrt_detached_voxels_device(0, lo, hi, 26, 0, 0, 0, &n);\n'
                   '    return a == VXRT_E_INVALID && b == VXRT_E_INVALID ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)


def test_both_libraries_export_them_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    for lib in (_build.LIB, H.variants_library()):
        out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
        for f in FUNCTIONS:
            assert f in exported, (lib, f)          # unmangled => extern "C"
    assert H.lib().vxrt_abi_version() == 6


def test_a_null_context_is_invalid(H):
    L = H.lib()
    pos = np.zeros((2, 3), np.int16)
    label = np.full(2, 0xABCD, np.uint32)
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = C.c_size_t(7)
    for connectivity in (6, 18, 26, 7, 0):
        conn = C.c_uint32(connectivity)
        assert L.vxrt_label_components_device(None, p(pos), C.c_size_t(2), conn, p(label), C.byref(n)) == H.E_INVALID
        assert L.vxrt_label_components_device(None, None, C.c_size_t(0), conn, None, C.byref(n)) == H.E_INVALID
        assert L.vxrt_label_components_device(None, None, C.c_size_t(0), conn, None, None) == H.E_INVALID
        assert L.vxrt_detached_voxels_device(None, lo, hi, conn, None, None, C.c_size_t(0), C.byref(n)) == H.E_INVALID
        assert L.vxrt_detached_voxels_device(None, None, None, conn, None, None, C.c_size_t(0), None) == H.E_INVALID
    assert n.value == 7 and (label == 0xABCD).all()


def test_the_new_sources_are_built_into_both_libraries():
    from gpu_voxel_raytracer_amd import _build
    csrc = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")
    for f in NEW_SOURCES:
        assert os.path.exists(os.path.join(csrc, f)), f
    assert "components.hip" in _build.SOURCES and "api_components.hip" in _build.SOURCES      # the variants build takes SOURCES too
    assert "components.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)


class NoLibrary:
    """Stands in for the loaded library: any call through it fails the test."""
    def __getattr__(self, name):
        raise AssertionError(f"{name} was called")


def bare_context(H):
    ctx = object.__new__(H.Context)      # no vxrt_create: the checks under test come before any library call
    ctx._L, ctx._h, ctx.device = NoLibrary(), None, 0
    return ctx


def test_the_wrapper_has_the_three_methods(H):
    assert list(inspect.signature(H.Context.label_components).parameters) == ["self", "pos", "connectivity"]
    assert list(inspect.signature(H.Context.detached_voxels).parameters) == ["self", "anchor_min", "anchor_max", "connectivity", "cap"]
    assert list(inspect.signature(H.Context.drop_detached).parameters) == ["self", "anchor_min", "anchor_max", "connectivity"]
    for f in (H.Context.label_components, H.Context.detached_voxels, H.Context.drop_detached):
        assert inspect.signature(f).parameters["connectivity"].default == 6


def test_the_wrappers_check_their_arguments_before_any_library_call(H):
    import torch
    ctx = bare_context(H)
    try:
        pos = np.zeros((5, 3), np.int16)
        for bad in (pos.astype(np.int32), pos.astype(np.uint16), pos.astype(np.float32), torch.zeros((5, 3), dtype=torch.int32)):
            with pytest.raises(ValueError):
                ctx.label_components(bad)                                 # dtype
        with pytest.raises(ValueError):
            ctx.label_components(np.zeros(10, np.int16))                  # not [n, 3]
        with pytest.raises(ValueError):
            ctx.label_components(torch.zeros((5, 3), dtype=torch.int16))  # a tensor of another device (the host's)
        for bad in (pos.tolist(), None, "pos"):
            with pytest.raises(TypeError):
                ctx.label_components(bad)
        for bad in (0, 7, 27, 8, -6, 6.0, "6", None, True):
            with pytest.raises(ValueError):
                ctx.label_components(pos, bad)
            with pytest.raises(ValueError):
                ctx.detached_voxels((0, 0, 0), (1, 1, 1), bad)
            with pytest.raises(ValueError):
                ctx.drop_detached((0, 0, 0), (1, 1, 1), connectivity=bad)
        for lo, hi in (((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 1, 1)), (None, (1, 1, 1)), ((0, 0, 0), None), (None, None)):
            with pytest.raises(ValueError):
                ctx.detached_voxels(lo, hi)
            with pytest.raises(ValueError):
                ctx.drop_detached(lo, hi)
        for cap in (-1, 2.5, "9", True):
            with pytest.raises(ValueError):
                ctx.detached_voxels((0, 0, 0), (1, 1, 1), cap=cap)
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


# ---- the model against a flood fill and against counts known by hand -----------------------------------------------------------------
def flood_labels(grid, connectivity):
    """grid: bool [a, b, c] -> int64 [a, b, c]: per occupied cell the least C-order index of its component (-1 where empty), by
    repeated minimum over the grid shifted by every offset until nothing changes.  Shifts go through a border of empty cells, so
    nothing wraps."""
    big = grid.size
    lab = np.where(grid, np.arange(big).reshape(grid.shape), big)
    offs = K.offsets(connectivity)
    while True:
        pad = np.pad(lab, 1, constant_values=big)
        best = lab.copy()
        for dx, dy, dz in offs:
            view = pad[1 + dx:1 + dx + grid.shape[0], 1 + dy:1 + dy + grid.shape[1], 1 + dz:1 + dz + grid.shape[2]]
            best = np.minimum(best, view)
        best = np.where(grid, best, big)
        if np.array_equal(best, lab):
            return np.where(grid, lab, -1)
        lab = best


@pytest.mark.parametrize("connectivity", K.CONNECTIVITIES)
@pytest.mark.parametrize("seed, dims, fill", [(1, (12, 12, 12), 0.30), (2, (12, 9, 5), 0.22), (3, (7, 12, 11), 0.45), (4, (12, 12, 1), 0.55)])
def test_the_model_equals_a_dense_flood_fill(seed, dims, fill, connectivity):
    rng = np.random.default_rng(seed)
    grid = rng.random(dims) < fill
    cells = np.argwhere(grid)                        # C order: the list index of a cell rises with its C-order grid index
    want = flood_labels(grid, connectivity)[grid]    # per listed cell, the least C-order grid index of its component
    grid_index = np.ravel_multi_index(tuple(cells.T), dims)
    got, count = K.label(cells - 5, connectivity)    # translated: the rule does not care
    assert np.array_equal(grid_index[got], want)
    assert count == len(np.unique(want))
    # a shuffled list with repeats: the same classes, each named by its least index
    order = rng.permutation(np.concatenate([np.arange(len(cells)), rng.integers(0, len(cells), len(cells) // 3)]))
    got2, count2 = K.label(cells[order] - 5, connectivity)
    assert count2 == count
    first = {}
    for i, w in enumerate(want[order].tolist()):
        first.setdefault(w, i)
    assert got2.tolist() == [first[w] for w in want[order].tolist()]


def test_hand_counts():
    board = np.argwhere(np.indices((16, 16, 16)).sum(axis=0) % 2 == 0)
    assert len(board) == 2048
    assert [K.label(board, c)[1] for c in K.CONNECTIVITIES] == [2048, 1, 1]
    pairs = {"face": ((3, 4, 5), (3, 5, 5), [1, 1, 1]), "edge": ((3, 4, 5), (4, 5, 5), [2, 1, 1]), "corner": ((3, 4, 5), (4, 3, 6), [2, 2, 1]),
             "apart": ((3, 4, 5), (5, 4, 5), [2, 2, 2]), "wrap": ((32767, 0, 0), (-32768, 0, 0), [2, 2, 2]),
             "wrap on every axis": ((32767, 32767, 32767), (-32768, -32768, -32768), [2, 2, 2]), "origin": ((-1, 0, 0), (0, 0, 0), [1, 1, 1]),
             "same": ((9, 9, 9), (9, 9, 9), [1, 1, 1])}
    for name, (a, b, counts) in pairs.items():
        for conn, want in zip(K.CONNECTIVITIES, counts):
            lab, count = K.label(np.array([a, b], np.int16), conn)
            assert count == want and lab.tolist() == ([0, 0] if want == 1 else [0, 1]), (name, conn)
    assert K.label(np.zeros((0, 3), np.int16), 6)[1] == 0


def test_the_models_detached_set():
    # a table: a top of 5 x 5 at y = 3 on one leg at (2, 0..2, 2); a loose voxel beside it, touching the top by a corner only
    cells = [(x, 3, z) for x in range(5) for z in range(5)] + [(2, y, 2) for y in range(3)] + [(5, 4, 5)]
    voxels = {c: (i % 128, 1, 2, 3) for i, c in enumerate(cells)}
    ground = ((-100, 0, -100), (100, 1, 100))
    assert [len(K.detached(voxels, *ground, c)[0]) for c in K.CONNECTIVITIES] == [1, 1, 0]
    pos, mrgb = K.detached(voxels, *ground, 6)
    assert pos.tolist() == [[5, 4, 5]] and mrgb.tolist() == [list(voxels[(5, 4, 5)])]
    del voxels[(2, 1, 2)]                                  # the leg is cut: the top and the leg's upper voxel fall
    pos, mrgb = K.detached(voxels, *ground, 26)
    assert len(pos) == 27 and (2, 0, 2) not in set(map(tuple, pos.tolist()))
    assert (np.diff(K.path_keys(pos)) > 0).all()           # ascending path order
    assert [tuple(b) for b in mrgb.tolist()] == [voxels[tuple(p)] for p in pos.tolist()]
    for empty in (((0, 0, 0), (0, 9, 9)), ((50, 50, 50), (60, 60, 60)), ((3, 3, 3), (2, 2, 2))):
        assert len(K.detached(voxels, *empty, 26)[0]) == len(voxels)      # an empty box, or one that misses: everything
    assert len(K.detached({}, *ground, 6)[0]) == 0
