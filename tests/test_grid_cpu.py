"""CPU: the dense-grid extension's interface (include/vxrt_grid.h) — plain C, declared, exported with C linkage, refused without a
context — and the Python model of grids (tests/grid_model.py): list -> grid -> list keeps the set, words <-> mrgb follows the
vxrt_set_voxels rule, and a grid's list builds the host builder's records."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import device_build_model as D
import grid_model as G
from conftest import ROOT


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vxrt_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_both_entry_points():
    assert declared("vxrt_grid.h") == ["vxrt_get_voxel_grid", "vxrt_set_voxel_grid"]
    assert len(declared("vxrt.h")) <= 40
    assert "vxrt_grid.h" in open(os.path.join(ROOT, "include", "vxrt.h")).read()
    assert '#include "vxrt_grid.h"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "vxrt_grid.h"\nint main(void) { return VXRT_GRID_PALETTE8 + VXRT_GRID_WORD32 == 3 ? 0 : 1; }\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)


def test_library_exports_both_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    assert "vxrt_set_voxel_grid" in exported and "vxrt_get_voxel_grid" in exported
    assert H.lib().vxrt_abi_version() == 6


def test_null_context_is_invalid(H):
    L = H.lib()
    dims = (C.c_uint32 * 3)(1, 1, 1)
    org = (C.c_int32 * 3)(0, 0, 0)
    cells = np.zeros(1, np.uint32)
    assert L.vxrt_set_voxel_grid(None, cells.ctypes.data_as(C.c_void_p), C.c_int(H.GRID_WORD32), dims, org, None) == H.E_INVALID
    assert L.vxrt_set_voxel_grid(None, None, C.c_int(H.GRID_WORD32), (C.c_uint32 * 3)(0, 0, 0), org, None) == H.E_INVALID
    assert L.vxrt_get_voxel_grid(None, org, dims, cells.ctypes.data_as(C.c_void_p)) == H.E_INVALID


def test_words_and_mrgb_follow_the_set_voxels_rule():
    rng = np.random.default_rng(1)
    mrgb = rng.integers(0, 256, (1000, 4)).astype(np.uint8)
    w = G.words_of(mrgb)
    assert np.all(w >> 31 == 1)
    assert np.array_equal(w, (0x80000000 | (mrgb[:, 0].astype(np.uint32) & 0x7F) << 24 | mrgb[:, 1].astype(np.uint32) << 16
                              | mrgb[:, 2].astype(np.uint32) << 8 | mrgb[:, 3]).astype(np.uint32))
    back = G.mrgb_of(w)
    assert np.array_equal(back[:, 1:], mrgb[:, 1:]) and np.array_equal(back[:, 0], mrgb[:, 0] & 0x7F)
    assert np.array_equal(G.words_of(back), w)


def as_set(pos, mrgb):
    return {(tuple(p), int(w)) for p, w in zip(np.asarray(pos, np.int64).tolist(), G.words_of(mrgb).tolist())}


def test_list_grid_list_round_trip():
    rng = np.random.default_rng(2)
    pos = np.unique(rng.integers(-40, 40, (3000, 3)), axis=0).astype(np.int16)
    mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    origin, dims = G.bounding_box(pos)
    grid = G.list_to_grid(pos, mrgb, origin, dims)
    assert grid.shape == dims and grid.dtype == np.int32
    p2, m2 = G.grid_to_list(grid, origin)
    assert as_set(p2, m2) == as_set(pos, mrgb)
    # a box that cuts the list keeps exactly the voxels inside it
    o2, d2 = (-5, 0, -40), (30, 7, 50)
    p3, m3 = G.grid_to_list(G.list_to_grid(pos, mrgb, o2, d2), o2)
    inside = np.all((pos >= o2) & (pos < np.add(o2, d2)), axis=1)
    assert as_set(p3, m3) == as_set(pos[inside], mrgb[inside])


def test_palette_grid_round_trip_and_records(H):
    rng = np.random.default_rng(3)
    pos = np.unique(rng.integers(-20, 30, (2000, 3)), axis=0).astype(np.int16)
    colours = rng.integers(0, 256, (40, 4)).astype(np.uint8)
    mrgb = colours[rng.integers(0, 40, len(pos))]
    origin, dims = G.bounding_box(pos)
    idx, palette = G.palette_grid(pos, mrgb, origin, dims)
    p2, m2 = G.grid_to_list(idx, origin, palette)
    assert as_set(p2, m2) == as_set(pos, mrgb)
    svo, _, leaves, depth = H.build_records(p2, m2)
    msvo, mleaves, mdepth = D.build(pos, mrgb)
    assert mdepth == depth and np.array_equal(msvo, svo) and np.array_equal(mleaves, leaves)
    many = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    assert G.palette_grid(pos, many, origin, dims) is None
