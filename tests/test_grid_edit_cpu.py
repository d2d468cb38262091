"""CPU: the grid-edit extension's interface (include/vxrt_grid_edit.h) — plain C, declared, exported with C linkage, refused without a
device — and the numpy model of a grid edit (tests/grid_edit_model.py) against a per-cell restatement of the header's definition."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edit_model as M
import grid_edit_model as GE
from conftest import ROOT


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vxrt_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_exactly_the_entry_point():
    assert declared("vxrt_grid_edit.h") == ["vxrt_edit_voxel_grid"]
    assert "vxrt_edit_voxel_grid" not in declared("vxrt.h") + declared("vxrt_grid.h") + declared("vxrt_edit.h")
    assert '#include "vxrt_grid.h"' in open(os.path.join(ROOT, "include", "vxrt_grid_edit.h")).read()
    assert '#include "vxrt_grid_edit.h"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "vxrt_grid_edit.h"\n'
                   'int main(void) {\n'
                   '    vxrt_grid_edit_counts n = {0, 0};\n'
                   '    vxrt_grid_edit_mode m = VXRT_GRID_EDIT_CLEAR;\n'
                   '    return VXRT_GRID_EDIT_REPLACE + VXRT_GRID_EDIT_SET == 3 && m == 3 && n.set + n.cleared == 0 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)


def test_library_exports_it_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    assert "vxrt_edit_voxel_grid" in exported
    assert H.lib().vxrt_abi_version() == 6


def test_null_and_bad_arguments_are_invalid_without_a_device(H):
    L = H.lib()
    dims = (C.c_uint32 * 3)(1, 1, 1)
    org = (C.c_int32 * 3)(0, 0, 0)
    cells = np.zeros(1, np.uint32)
    pal = np.zeros((256, 4), np.uint8)
    counts = (C.c_uint64 * 2)(7, 7)
    p = cells.ctypes.data_as(C.c_void_p)
    f = L.vxrt_edit_voxel_grid
    assert f(None, p, C.c_int(H.GRID_WORD32), dims, org, None, C.c_int(1), counts) == H.E_INVALID
    assert list(counts) == [0, 0]
    assert f(None, p, C.c_int(H.GRID_WORD32), dims, org, None, C.c_int(1), None) == H.E_INVALID
    assert f(None, None, C.c_int(H.GRID_WORD32), (C.c_uint32 * 3)(0, 0, 0), org, None, C.c_int(1), None) == H.E_INVALID
    assert f(None, p, C.c_int(H.GRID_PALETTE8), dims, org, pal.ctypes.data_as(C.c_void_p), C.c_int(3), None) == H.E_INVALID
    assert f(None, p, C.c_int(H.GRID_WORD32), None, org, None, C.c_int(1), None) == H.E_INVALID
    assert f(None, p, C.c_int(H.GRID_WORD32), dims, None, None, C.c_int(1), None) == H.E_INVALID
    assert f(None, p, C.c_int(9), dims, org, None, C.c_int(1), None) == H.E_INVALID
    assert f(None, p, C.c_int(H.GRID_WORD32), dims, org, None, C.c_int(0), None) == H.E_INVALID
    assert (H.GRID_EDIT_REPLACE, H.GRID_EDIT_SET, H.GRID_EDIT_CLEAR) == (GE.REPLACE, GE.SET, GE.CLEAR)


def brute_force(model, cells, origin, mode, depth, palette=None):
    """The header's definition cell by cell: s(p), g(p), the two lists, then clears and sets applied as vxrt_edit_voxels would."""
    cells = np.asarray(cells)
    h = 1 << depth
    clears, sets = [], []
    for i, j, k in np.ndindex(*cells.shape):
        p = (origin[0] + i, origin[1] + j, origin[2] + k)
        c = int(cells[i, j, k])
        if cells.dtype == np.uint8:
            g = M.word(palette[c]) if c else 0
        else:
            g = int(np.int32(c)) if (c & 0xFFFFFFFF) >> 31 else 0
        if not all(-h <= v < h for v in p):
            if g and mode != GE.CLEAR:
                raise GE.OutsideCube()
            continue
        s = model.get(p, 0)
        empties = (mode == GE.REPLACE and g == 0) or (mode == GE.CLEAR and g != 0)
        if s != 0 and empties:
            clears.append(p)
        if mode in (GE.SET, GE.REPLACE) and g != 0 and s != g:
            sets.append((p, g))
    out = dict(model)
    for p in clears:
        del out[p]
    for p, g in sets:
        out[p] = g
    return sorted(clears), sorted(sets), out


@pytest.mark.parametrize("seed", range(12))
def test_model_equals_the_per_cell_definition(seed):
    rng = np.random.default_rng(seed)
    depth = int(rng.integers(0, 5))
    h = 1 << depth
    palette = rng.integers(0, 256, (256, 4)).astype(np.uint8)
    # a scene in its root cube whose words partly match the grid's: the palette's words and a few others
    n = int(rng.integers(0, (2 * h) ** 3 // 2 + 2))
    pos = rng.integers(-h, h, (n, 3))
    words = [M.word(palette[rng.integers(1, 256)]) if rng.random() < 0.5 else M.word(rng.integers(0, 256, 4)) for _ in range(n)]
    model = {tuple(p): w for p, w in zip(pos.tolist(), words)}
    dims = tuple(int(v) for v in rng.integers(1, 2 * h + 4, 3))
    origin = tuple(int(v) for v in rng.integers(-h - 3, h, 3))
    for fmt in ("palette8", "word32"):
        if fmt == "palette8":
            cells = np.where(rng.random(dims) < 0.5, rng.integers(1, 256, dims), 0).astype(np.uint8)
            pal = palette
        else:
            occ = rng.random(dims) < 0.5
            from_scene = np.array([model.get((origin[0] + i, origin[1] + j, origin[2] + k), 0) for i, j, k in np.ndindex(*dims)],
                                  np.int64).reshape(dims)
            w = np.where(rng.random(dims) < 0.5, from_scene, rng.integers(0, 1 << 31, dims) | (1 << 31))
            w = np.where(w == 0, rng.integers(0, 1 << 31, dims) | (1 << 31), w)
            cells = np.where(occ, w, rng.integers(0, 1 << 31, dims)).astype(np.int64).astype(np.uint32).view(np.int32)  # junk below bit 31
            pal = None
        for mode in (GE.REPLACE, GE.SET, GE.CLEAR):
            try:
                want = brute_force(model, cells, origin, mode, depth, pal)
            except GE.OutsideCube:
                with pytest.raises(GE.OutsideCube):
                    GE.edit_lists(model, cells, origin, mode, depth, pal)
                continue
            cpos, spos, swords, out = GE.edit_lists(model, cells, origin, mode, depth, pal)
            assert sorted(map(tuple, cpos.tolist())) == want[0], (seed, fmt, mode)
            assert sorted(zip(map(tuple, spos.tolist()), swords.tolist())) == want[1], (seed, fmt, mode)
            assert out == want[2], (seed, fmt, mode)
            # the edit model's two calls give the same dict, and the words survive the trip through (material, r, g, b)
            twin = dict(model)
            if len(cpos):
                M.apply(twin, cpos, None)
            if len(spos):
                M.apply(twin, spos, GE.mrgb_of_words(swords))
            assert twin == out, (seed, fmt, mode)


def test_inside_cells_only_and_outside_rules():
    model = {(0, 0, 0): M.word((1, 2, 3, 4))}
    cells = np.zeros((4, 1, 1), np.uint32)
    cells[3, 0, 0] = 0x80000001   # p = (2, 0, 0): outside the root cube of depth 1 ([-2, 2))
    cells = cells.view(np.int32)
    with pytest.raises(GE.OutsideCube):
        GE.edit_lists(model, cells, (-1, 0, 0), "set", 1)
    with pytest.raises(GE.OutsideCube):
        GE.edit_lists(model, cells, (-1, 0, 0), "replace", 1)
    c, s, w, out = GE.edit_lists(model, cells, (-1, 0, 0), "clear", 1)
    assert len(c) == 0 and len(s) == 0 and out == model
    c, s, w, out = GE.edit_lists(model, cells[:3], (-1, 0, 0), "replace", 1)   # empty cells clear the voxel at 0
    assert c.tolist() == [[0, 0, 0]] and len(s) == 0 and out == {}
