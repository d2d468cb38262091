"""CPU: the component table's interface (include/vxrt_pieces.h) — plain C, declared, exported with C linkage by both libraries, refused
without a context — the Python wrappers' argument checks, which run before any library call, and the model of rules 6 to 9
(pieces_model.py) against something that does not follow its wording: the flood fill on a dense grid of test_components_cpu.py for
the labels, then numpy per label for count, bounds and sums, and tables known by hand."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import components_model as K
import pieces_model as P
from conftest import ROOT
from test_components_cpu import bare_context, declared, flood_labels

FUNCTIONS = ["vxrt_component_table_device", "vxrt_detached_pieces_device"]
HEADER = "vxrt_pieces.h"
NEW_SOURCES = ("pieces.hip", "api_pieces.hip", "pieces.h")


def test_header_declares_exactly_the_two_entry_points():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt.h"' in text and '#include "vxrt_components.h"' in text
    assert "distinct positions" in text and "ascending label" in text
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", hdr], capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text('#include <stddef.h>\n'
                   f'#include "{HEADER}"\n'
                   'typedef char size_is_48[sizeof(vxrt_piece) == 48 ? 1 : -1];\n'
                   'typedef char sum_is_at_24[offsetof(vxrt_piece, sum) == 24 ? 1 : -1];\n'
                   'typedef char min_is_at_8[offsetof(vxrt_piece, min) == 8 && offsetof(vxrt_piece, max) == 14 ? 1 : -1];\n'
                   'int main(void) {\n'
                   '    size_t n = 0, k = 0;\n'
                   '    const int32_t lo[3] = {0, 0, 0}, hi[3] = {1, 1, 1};\n'
                   '    int a = vxrt_component_table_device(0, 0, 0, 6, 0, 0, 0, 0, &n);\n'
                   '    int b = vxrt_detached_pieces_device(0, lo, hi, 26, 0, UINT32_MAX, 0, 0, 0, 0, &n, 0, 0, &k);\n'
                   '    return a == VXRT_E_INVALID && b == VXRT_E_INVALID ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "vxrt.hpp"\nstatic_assert(sizeof(vxrt_piece) == 48 && alignof(vxrt_piece) == 8, "vxrt_piece");\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cpp)], check=True)


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
    label, ids = np.full(2, 0xABCD, np.uint32), np.full(2, 0xABCD, np.uint32)
    info = np.full(2 * P.PIECE.itemsize, 0x5A, np.uint8)
    lo, hi = (C.c_int32 * 3)(0, 0, 0), (C.c_int32 * 3)(4, 4, 4)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n, k = C.c_size_t(7), C.c_size_t(9)
    two, none, every = C.c_size_t(2), C.c_size_t(0), C.c_uint32(0xFFFFFFFF)
    for connectivity in (6, 18, 26, 7, 0):
        conn = C.c_uint32(connectivity)
        assert L.vxrt_component_table_device(None, p(pos), two, conn, p(label), p(ids), p(info), two, C.byref(n)) == H.E_INVALID
        assert L.vxrt_component_table_device(None, None, none, conn, None, None, None, none, C.byref(n)) == H.E_INVALID
        assert L.vxrt_component_table_device(None, None, none, conn, None, None, None, none, None) == H.E_INVALID
        assert L.vxrt_detached_pieces_device(None, lo, hi, conn, C.c_uint32(0), every, p(pos), p(label), p(ids), two, C.byref(n), p(info), two,
                                             C.byref(k)) == H.E_INVALID
        assert L.vxrt_detached_pieces_device(None, lo, hi, conn, C.c_uint32(0), every, None, None, None, none, C.byref(n), None, none,
                                             C.byref(k)) == H.E_INVALID
        assert L.vxrt_detached_pieces_device(None, None, None, conn, C.c_uint32(0), every, None, None, None, none, None, None, none, None) == H.E_INVALID
    assert n.value == 7 and k.value == 9 and (label == 0xABCD).all() and (ids == 0xABCD).all() and (info == 0x5A).all() and not pos.any()


def test_the_new_sources_are_built_into_both_libraries():
    from gpu_voxel_raytracer_amd import _build
    csrc = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")
    for f in NEW_SOURCES:
        assert os.path.exists(os.path.join(csrc, f)), f
    assert "pieces.hip" in _build.SOURCES and "api_pieces.hip" in _build.SOURCES      # the variants build takes SOURCES too
    assert "pieces.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)


def test_the_wrapper_has_the_three_methods(H):
    selection = ["self", "anchor_min", "anchor_max", "connectivity", "min_voxels", "max_voxels", "cap"]
    assert list(inspect.signature(H.Context.component_table).parameters) == ["self", "pos", "connectivity"]
    assert list(inspect.signature(H.Context.detached_pieces).parameters) == selection
    assert list(inspect.signature(H.Context.drop_detached_pieces).parameters) == selection
    for f in (H.Context.component_table, H.Context.detached_pieces, H.Context.drop_detached_pieces):
        assert inspect.signature(f).parameters["connectivity"].default == 6
    for f in (H.Context.detached_pieces, H.Context.drop_detached_pieces):
        defaults = {name: prm.default for name, prm in inspect.signature(f).parameters.items()}
        assert (defaults["min_voxels"], defaults["max_voxels"], defaults["cap"]) == (0, None, None)


def test_the_wrappers_check_their_arguments_before_any_library_call(H):
    import torch
    ctx = bare_context(H)
    box = ((0, 0, 0), (1, 1, 1))
    try:
        pos = np.zeros((5, 3), np.int16)
        for bad in (pos.astype(np.int32), pos.astype(np.uint16), pos.astype(np.float32), torch.zeros((5, 3), dtype=torch.int32)):
            with pytest.raises(ValueError):
                ctx.component_table(bad)                                 # dtype
        with pytest.raises(ValueError):
            ctx.component_table(np.zeros(10, np.int16))                  # not [n, 3]
        with pytest.raises(ValueError):
            ctx.component_table(torch.zeros((5, 3), dtype=torch.int16))  # a tensor of another device (the host's)
        for bad in (pos.tolist(), None, "pos"):
            with pytest.raises(TypeError):
                ctx.component_table(bad)
        for method in (ctx.detached_pieces, ctx.drop_detached_pieces):
            for bad in (0, 7, 27, 8, -6, 6.0, "6", None, True):
                with pytest.raises(ValueError):
                    method(*box, bad)
            for lo, hi in (((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1, 1, 1)), (None, (1, 1, 1)), ((0, 0, 0), None), (None, None)):
                with pytest.raises(ValueError):
                    method(lo, hi)
            for cap in (-1, 2.5, "9", True):
                with pytest.raises(ValueError):
                    method(*box, cap=cap)
            for bad in (-1, 1 << 32, 2.0, "3", True):
                with pytest.raises(ValueError):
                    method(*box, max_voxels=bad)
                with pytest.raises(ValueError):
                    method(*box, min_voxels=bad)
            with pytest.raises(ValueError):
                method(*box, min_voxels=None)
        for bad in (0, 7, 27, 8, -6, 6.0, "6", None, True):
            with pytest.raises(ValueError):
                ctx.component_table(pos, bad)
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


# ---- the model against a flood fill plus numpy, and against tables known by hand ---------------------------------------------------
def assert_tables_equal(got, want, what):
    assert got.dtype == P.PIECE and want.dtype == P.PIECE and len(got) == len(want), (what, len(got), len(want))
    for f in P.FIELDS + ("reserved",):
        assert np.array_equal(got[f], want[f]), (what, f)


@pytest.mark.parametrize("connectivity", K.CONNECTIVITIES)
@pytest.mark.parametrize("seed, dims, fill", [(1, (12, 12, 12), 0.30), (2, (12, 9, 5), 0.22), (3, (7, 12, 11), 0.45), (4, (12, 12, 1), 0.55)])
def test_the_model_equals_a_dense_flood_fill(seed, dims, fill, connectivity):
    rng = np.random.default_rng(seed)
    grid = rng.random(dims) < fill
    cells = np.argwhere(grid)
    dense = flood_labels(grid, connectivity)[grid]            # per listed cell, the least C-order grid index of its component
    order = rng.permutation(np.concatenate([np.arange(len(cells)), rng.integers(0, len(cells), len(cells) // 3)]))
    for shift, pick in ((-5, np.arange(len(cells))), (32767 - 11, order)):      # in C order; shuffled with repeats, ending at 32767
        pos, comp = cells[pick] + shift, dense[pick]
        label, ids, table = P.component_table(pos, connectivity)
        first = {}
        for i, w in enumerate(comp.tolist()):
            first.setdefault(w, i)
        want_label = np.array([first[w] for w in comp.tolist()])
        assert np.array_equal(label, want_label)
        firsts = np.unique(want_label)                            # ascending: the numbering
        assert np.array_equal(ids, np.searchsorted(firsts, want_label)) and np.array_equal(table["first"], firsts)
        assert not table["reserved"].any()
        for c, f in enumerate(firsts.tolist()):
            mine = np.unique(pos[want_label == f], axis=0)        # distinct positions
            assert table["voxels"][c] == len(mine)
            assert np.array_equal(table["min"][c], mine.min(axis=0)) and np.array_equal(table["max"][c], mine.max(axis=0))
            assert np.array_equal(table["sum"][c], mine.sum(axis=0))
    # the scene rule on the same grid: a voxel dict, the anchor box its lowest x layer
    voxels = {tuple(c): (i % 128, 1, 2, 3) for i, c in enumerate(cells.tolist())}
    anchor = ((0, -100, -100), (1, 100, 100))
    held = set(dense[cells[:, 0] == 0].tolist())
    loose = np.array([w not in held for w in dense.tolist()])
    sizes = {w: int((dense == w).sum()) for w in set(dense[loose].tolist())}
    for lo, hi in ((0, P.EVERY), (2, 5), (1, 1), (6, P.EVERY), (5, 2)):
        pos, mrgb, piece, table = P.detached_pieces(voxels, *anchor, connectivity, lo, hi)
        keep = np.array([l and lo <= sizes[w] <= hi for l, w in zip(loose.tolist(), dense.tolist())], bool)
        assert sorted(map(tuple, pos.tolist())) == sorted(map(tuple, cells[keep].tolist())), (lo, hi)
        assert (np.diff(K.path_keys(pos)) > 0).all() and [tuple(b) for b in mrgb.tolist()] == [voxels[tuple(q)] for q in pos.tolist()]
        assert len(table) == len({w for w, k in zip(dense.tolist(), keep.tolist()) if k})
        if lo == 0 and hi == P.EVERY:
            d_pos, d_mrgb = K.detached(voxels, *anchor, connectivity)
            assert np.array_equal(pos, d_pos) and np.array_equal(mrgb, d_mrgb)      # the full range is the detached set
        _, ids, again = P.component_table(pos, connectivity)                        # the identity the header states
        assert np.array_equal(piece, ids)
        assert_tables_equal(table, again, (lo, hi))


def row(first, voxels, lo, hi, total):
    r = np.zeros((), P.PIECE)
    r["first"], r["voxels"], r["min"], r["max"], r["sum"] = first, voxels, lo, hi, total
    return r


def test_hand_tables():
    pairs = {"face": ((3, 4, 5), (3, 5, 5), [1, 1, 1]), "edge": ((3, 4, 5), (4, 5, 5), [2, 1, 1]), "corner": ((3, 4, 5), (4, 3, 6), [2, 2, 1])}
    for name, (a, b, counts) in pairs.items():
        for conn, want in zip(K.CONNECTIVITIES, counts):
            label, ids, table = P.component_table([a, b], conn)
            if want == 1:
                both = np.array([a, b])
                expect = np.array([row(0, 2, both.min(axis=0), both.max(axis=0), both.sum(axis=0))])
                assert (label.tolist(), ids.tolist()) == ([0, 0], [0, 0]), (name, conn)
            else:
                expect = np.array([row(0, 1, a, a, a), row(1, 1, b, b, b)])
                assert (label.tolist(), ids.tolist()) == ([0, 1], [0, 1]), (name, conn)
            assert_tables_equal(table, expect, (name, conn))
    for a, b in (((32767, 0, 0), (-32768, 0, 0)), ((-32768, -32768, -32768), (32767, 32767, 32767))):      # nothing wraps
        for conn in K.CONNECTIVITIES:
            label, ids, table = P.component_table([a, b], conn)
            assert_tables_equal(table, np.array([row(0, 1, a, a, a), row(1, 1, b, b, b)]), (a, b, conn))
            assert np.array_equal(table["min"], table["max"]) and ids.tolist() == [0, 1]
    # a position listed four times counts once; numbering is by label, not by position
    label, ids, table = P.component_table([(9, 9, 9), (-4, 0, 0), (9, 9, 9), (9, 9, 9), (-5, 0, 0), (9, 9, 9)], 6)
    assert label.tolist() == [0, 1, 0, 0, 1, 0] and ids.tolist() == [0, 1, 0, 0, 1, 0]
    assert_tables_equal(table, np.array([row(0, 1, (9, 9, 9), (9, 9, 9), (9, 9, 9)), row(1, 2, (-5, 0, 0), (-4, 0, 0), (-9, 0, 0))]), "repeats")
    label, ids, table = P.component_table(np.zeros((0, 3), np.int16), 26)
    assert len(label) == len(ids) == len(table) == 0
    board = np.argwhere(np.indices((16, 16, 16)).sum(axis=0) % 2 == 0)
    assert [len(P.component_table(board, c)[2]) for c in K.CONNECTIVITIES] == [2048, 1, 1]
    one = P.component_table(board, 18)[2][0]
    assert one["voxels"] == 2048 and one["min"].tolist() == [0, 0, 0] and one["max"].tolist() == [15, 15, 15] and one["sum"].tolist() == board.sum(axis=0).tolist()


def test_the_models_detached_pieces():
    # test_components_cpu's table with its leg cut, a loose voxel beside it and a crumb of two further off
    cells = [(x, 3, z) for x in range(5) for z in range(5)] + [(2, 0, 2), (2, 2, 2)] + [(5, 4, 5)] + [(9, 9, 9), (9, 9, 10)]
    voxels = {c: (i % 128, 1, 2, 3) for i, c in enumerate(cells)}
    ground = ((-100, 0, -100), (100, 1, 100))
    sizes = {6: [26, 1, 2], 18: [26, 1, 2], 26: [27, 2]}
    for conn in K.CONNECTIVITIES:
        pos, mrgb, piece, table = P.detached_pieces(voxels, *ground, conn)
        assert table["voxels"].tolist() == sizes[conn] and len(pos) == sum(sizes[conn]) and (2, 0, 2) not in set(map(tuple, pos.tolist()))
        assert table["first"].tolist() == [int(np.nonzero(piece == c)[0][0]) for c in range(len(table))]
        assert (np.diff(table["first"].astype(np.int64)) > 0).all()
        small = P.detached_pieces(voxels, *ground, conn, 0, 2)
        assert small[3]["voxels"].tolist() == [s for s in sizes[conn] if s <= 2] and small[3]["first"][0] == 0
        assert len(P.detached_pieces(voxels, *ground, conn, 3, 25)[0]) == 0 and len(P.detached_pieces(voxels, *ground, conn, 5, 2)[3]) == 0
    assert len(P.detached_pieces({}, *ground, 6)[0]) == 0
