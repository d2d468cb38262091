"""CPU: the distance interface (include/vxrt_distance.h) — plain C, declared once, exported with C linkage by both libraries, refused
without a context — the Python wrappers' signatures and argument checks, which run before any library call; the rule's model
(distance_model.py) against a dense numpy statement, against counts known by hand and against the identities the modes must
satisfy, morph_model's among them; and the kernels' own arithmetic (csrc/distance_rule.h: the rank, the radius, the nearest bit of a
row, the two bounded minima, the tile's path index, the tile key's neighbour, the walks), compiled by g++ with the
undefined-behaviour and address sanitizers into a program of its own that does what a block does, tile by tile and thread by
thread, in arrays of exactly the kernel's sizes, against the model."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import distance_model as D
import morph_model as M
import transform_model as T
from conftest import ROOT
from test_components_cpu import bare_context, declared
from test_morph_cpu import SANITIZED

FUNCTIONS = ["vxrt_distance_voxels_device"]
HEADER = "vxrt_distance.h"
NEW_SOURCES = ("distance.hip", "api_distance.hip", "distance.h", "distance_rule.h")
CSRC = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")


# ---- the header, the libraries, the wrappers ---------------------------------------------------------------------------------------
def test_header_declares_exactly_the_one_entry_point():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt.h"' in text and "typedef enum vxrt_distance_mode" in text
    assert "last entry of a position wins" in text and "bit 7" in text and "path order" in text and "do not wrap" in text
    assert "rank(-k) = 2k - 1" in text and "SQUARED" in text
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    assert "api_distance.hip" in open(os.path.join(CSRC, "ctx.h")).read()
    assert len(declared("vxrt.h")) <= 40


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), hdr],
                         capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text(f'#include "{HEADER}"\n'
                   'typedef char modes_are_0_to_3[VXRT_DISTANCE_DEPTH == 0 && VXRT_DISTANCE_FIELD == 1 && VXRT_DISTANCE_ERODE == 2 && VXRT_DISTANCE_DILATE == 3 ? 1 : -1];\n'
                   'typedef char limits[VXRT_DISTANCE_FAR == 0xFFFFu && VXRT_DISTANCE_MAX_D2 == 256u ? 1 : -1];\n'
                   'int main(void) {\n'
                   '    size_t n = 7;\n'
                   '    vxrt_distance_mode mode = VXRT_DISTANCE_FIELD;\n'
                   '    int rc = vxrt_distance_voxels_device(0, 0, 0, 0, (uint32_t)mode, 9, 0, 0, 0, 0, &n);\n'
                   '    return rc == VXRT_E_INVALID && n == 7 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "vxrt.hpp"\n'
                   'size_t f(vxrt::Context& c, const int16_t (*p)[3], const uint8_t (*m)[4], int16_t (*q)[3], uint8_t (*w)[4], uint16_t* d) {\n'
                   '    return c.distance_voxels_device(p, nullptr, 1, VXRT_DISTANCE_ERODE, 4) + c.distance_voxels_device(p, m, 1, VXRT_DISTANCE_DILATE, 256, q, w, d, 27); }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(cpp)], check=True)


def test_both_libraries_export_it_with_c_linkage(H):
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
    mrgb = np.full((2, 4), 9, np.uint8)
    out_pos = np.full((64, 3), 0x5A5A, np.uint16)
    out_mrgb = np.full((64, 4), 0xA5, np.uint8)
    out_d2 = np.full(64, 0x3C3C, np.uint16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = C.c_size_t(7)
    for count in (2, 0, 1 << 32):
        k = C.c_size_t(count)
        for mode, max_d2 in ((0, 1), (3, 256), (4, 1), (1, 0), (2, 257)):
            args = (C.c_uint32(mode), C.c_uint32(max_d2))
            assert L.vxrt_distance_voxels_device(None, p(pos), p(mrgb), k, *args, p(out_pos), p(out_mrgb), p(out_d2), C.c_size_t(64), C.byref(n)) == H.E_INVALID
            assert L.vxrt_distance_voxels_device(None, p(pos), None, k, *args, None, None, None, C.c_size_t(0), C.byref(n)) == H.E_INVALID
            assert L.vxrt_distance_voxels_device(None, None, None, k, *args, None, None, None, C.c_size_t(0), None) == H.E_INVALID
    assert b"null context" in L.vxrt_last_error()
    assert n.value == 7 and (out_pos == 0x5A5A).all() and (out_mrgb == 0xA5).all() and (out_d2 == 0x3C3C).all() and not pos.any() and (mrgb == 9).all()


def test_the_new_sources_are_built_into_both_libraries():
    from gpu_voxel_raytracer_amd import _build
    for f in NEW_SOURCES:
        assert os.path.exists(os.path.join(CSRC, f)), f
    assert "distance.hip" in _build.SOURCES and "api_distance.hip" in _build.SOURCES      # the variants build takes SOURCES too
    assert "distance.h" in _build.HEADERS and "distance_rule.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)
    rule = open(os.path.join(CSRC, "distance_rule.h")).read()
    assert "#include <hip" not in rule and '#include "' not in rule           # nothing from HIP, nothing of the project's


def test_the_wrapper_signatures_and_constants(H):
    params = inspect.signature(H.Context.distance_voxels).parameters
    assert list(params) == ["self", "pos", "mrgb", "mode", "max_d2", "cap"] and params["cap"].default is None
    for f in (H.Context.depth_voxels, H.Context.dilate_ball, H.Context.erode_ball, H.Context.margin_ball, H.Context.close_ball, H.Context.open_ball):
        assert list(inspect.signature(f).parameters) == ["self", "pos", "mrgb", "max_d2"], f
    assert (H.DISTANCE_DEPTH, H.DISTANCE_FIELD, H.DISTANCE_ERODE, H.DISTANCE_DILATE) == (0, 1, 2, 3) == D.MODES
    assert (H.DISTANCE_FAR, H.DISTANCE_MAX_D2) == (0xFFFF, 256) == (D.FAR, D.MAX_D2)


def test_the_wrappers_check_their_arguments_before_any_library_call(H):
    import torch
    ctx = bare_context(H)
    try:
        pos, mrgb = np.zeros((5, 3), np.int16), np.zeros((5, 4), np.uint8)
        calls = (lambda p, c, max_d2=4: ctx.distance_voxels(p, c, H.DISTANCE_DILATE, max_d2), lambda p, c, max_d2=4: ctx.depth_voxels(p, c, max_d2),
                 lambda p, c, max_d2=4: ctx.dilate_ball(p, c, max_d2), lambda p, c, max_d2=4: ctx.erode_ball(p, c, max_d2),
                 lambda p, c, max_d2=4: ctx.margin_ball(p, c, max_d2), lambda p, c, max_d2=4: ctx.close_ball(p, c, max_d2),
                 lambda p, c, max_d2=4: ctx.open_ball(p, c, max_d2))
        for call in calls:
            for bad in (pos.astype(np.int32), pos.astype(np.uint16), pos.astype(np.float32), torch.zeros((5, 3), dtype=torch.int32), np.zeros(15, np.int16),
                        np.zeros((5, 4), np.int16), torch.zeros((5, 3), dtype=torch.int16), torch.zeros((3, 5), dtype=torch.int16).t()):
                with pytest.raises(ValueError):
                    call(bad, None)
            for bad in (mrgb.astype(np.int8), mrgb.astype(np.uint32), np.zeros((5, 3), np.uint8), np.zeros(20, np.uint8), np.zeros((4, 4), np.uint8),
                        torch.zeros((5, 4), dtype=torch.uint8), torch.zeros((4, 5), dtype=torch.uint8).t()):
                with pytest.raises(ValueError):
                    call(pos, bad)                                         # ... before anything is uploaded
            for bad in (pos.tolist(), None, "pos"):
                with pytest.raises(TypeError):
                    call(bad, None)
            with pytest.raises(TypeError):
                call(pos, mrgb.tolist())
            for bad in (0, 257, -1, 4.0, "4", None, True):
                with pytest.raises(ValueError):
                    call(pos, mrgb, bad)
        for bad in (-1, 4, 1.0, "0", None, True):
            with pytest.raises(ValueError):
                ctx.distance_voxels(pos, mrgb, bad, 4)
        for bad in (-1, 1.5, "3", True):
            with pytest.raises(ValueError):
                ctx.distance_voxels(pos, mrgb, H.DISTANCE_ERODE, 4, cap=bad)
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


# ---- the model -------------------------------------------------------------------------------------------------------------------
def as_dict(pos, mrgb, d2):
    bytes_ = [None] * len(pos) if mrgb is None else [tuple(b) for b in mrgb.tolist()]
    return {tuple(p): (b, d) for p, b, d in zip(pos.tolist(), bytes_, d2.tolist())}


def equal(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def test_rank_radius_and_the_offsets():
    assert [D.rank(d) for d in (0, -1, 1, -2, 2, -16, 16)] == [0, 1, 2, 3, 4, 31, 32]
    assert [D.radius(m) for m in (1, 2, 3, 4, 8, 9, 15, 16, 255, 256)] == [1, 1, 1, 2, 2, 3, 3, 4, 15, 16]
    assert D.offsets(1) == ((0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
    assert [len(D.offsets(m)) for m in (1, 2, 3, 4, 5, 9, 255, 256)] == [7, 19, 27, 33, 57, 123, 17071, 17077]


def dense(grid, colour, mode, max_d2):
    """The modes on a dense occupancy grid (numpy; padded so that nothing reaches its border): a second, independent statement of
    rules 4 to 6.  The offsets are visited in ascending order of rule 5's key and the first writer of a cell wins."""
    pad = D.radius(max_d2) + 1
    occ = np.pad(grid, pad)
    col = np.pad(colour, [(pad, pad)] * 3 + [(0, 0)])

    def shifted(a, o):     # a'[x] = a[x + o]
        return np.roll(a, (-o[0], -o[1], -o[2]), axis=(0, 1, 2))

    target = ~occ if mode in (D.DEPTH, D.ERODE) else occ
    d2 = np.full(occ.shape, D.FAR, np.int64)
    src = col.copy()
    for o in D.offsets(max_d2):
        fresh = shifted(target, o) & (d2 == D.FAR)
        d2[fresh] = o[0] * o[0] + o[1] * o[1] + o[2] * o[2]
        src[fresh] = shifted(col, o)[fresh]
    if mode == D.DEPTH:
        keep, src = occ, col
    elif mode == D.ERODE:
        keep, src = occ & (d2 > max_d2), col
    elif mode == D.FIELD:
        keep = ~occ & (d2 <= max_d2)
    else:
        keep = d2 <= max_d2
    return {tuple((p - pad).tolist()): (tuple(src[tuple(p)].tolist()), int(d2[tuple(p)])) for p in np.argwhere(keep)}


@pytest.mark.parametrize("max_d2", (1, 2, 3, 4, 5, 9, 16, 17))
def test_the_model_against_a_dense_grid(max_d2):
    rng = np.random.default_rng(60 + max_d2)
    for side, density in ((5, 0.5), (8, 0.1), (10, 0.9)):                 # 10 + 2 (4 + 1) = 20 cells a side at the most
        grid = rng.random((side, side, side)) < density
        colour = rng.integers(0, 128, (side, side, side, 4)).astype(np.uint8)
        pos = np.argwhere(grid).astype(np.int16)
        mrgb = colour[grid]
        for mode in D.MODES:
            want = dense(grid, colour, mode, max_d2)
            assert as_dict(*D.distance(pos, mrgb, mode, max_d2)) == want, (side, D.NAMES[mode], max_d2)
            assert as_dict(*D.distance_np(pos, mrgb, mode, max_d2)) == want, (side, D.NAMES[mode], max_d2)


def test_counts_known_by_hand():
    one = np.array([[3, -4, 5]], np.int16)
    count = lambda pos, mode, max_d2, fn=D.distance_np: len(fn(pos, None, mode, max_d2)[0])        # noqa: E731
    assert [count(one, D.DILATE, m, D.distance) for m in (1, 2, 3, 4, 5, 9)] == [7, 19, 27, 33, 57, 123]
    assert [count(one, D.DILATE, m) for m in (1, 2, 3, 4, 5, 9, 255, 256)] == [7, 19, 27, 33, 57, 123, 17071, 17077]
    cube = M.cube16()[0]
    assert [count(cube, D.ERODE, m) for m in (1, 3, 4, 49, 63, 64)] == [2744, 2744, 1728, 8, 8, 0]
    assert [count(D.solid(31, -15)[0], D.ERODE, m) for m in (255, 256)] == [1, 0]
    pos, _, d2 = D.distance_np(D.solid(33, -16)[0], None, D.ERODE, 256)
    assert pos.tolist() == [[0, 0, 0]] and d2.tolist() == [D.FAR]
    pos, _, d2 = D.distance_np(D.solid(33, -16)[0], None, D.DEPTH, 256)
    assert len(pos) == 33 ** 3 and d2[(pos == 0).all(axis=1)].tolist() == [D.FAR] and d2[(pos == [1, 0, 0]).all(axis=1)].tolist() == [256]
    corner = np.array([[32767, 32767, 32767]], np.int16)
    for fn in (D.distance, D.distance_np):
        assert fn(corner, None, D.DEPTH, 3)[2].tolist() == [1] and count(corner, D.DILATE, 3, fn) == 8
        assert count(corner, D.ERODE, 256, fn) == 0


@pytest.fixture(scope="module")
def lists():
    rng = np.random.default_rng(3)
    pts = rng.integers(-4, 6, (500, 3)).astype(np.int16)              # 500 random points of a cube of 10^3: duplicates are certain
    return {"cube8": D.solid(8, -4), "shell": T.shell(3), "random": (pts, rng.integers(0, 256, (500, 4)).astype(np.uint8))}


def test_the_identities(lists):
    for name, (pos, mrgb) in lists.items():
        s = T.source_of(pos, mrgb)
        for max_d2 in (1, 2, 3, 6):
            depth, field, eroded, dilated = (as_dict(*D.distance_np(pos, mrgb, mode, max_d2)) for mode in D.MODES)
            near = {p: v for p, v in depth.items() if v[1] <= max_d2}
            assert not near.keys() & eroded.keys() and {**near, **eroded} == depth and depth.keys() == s.keys(), (name, max_d2)
            assert all(v == (s[p], D.FAR) for p, v in eroded.items())
            assert not field.keys() & s.keys() and {**field, **{p: (b, 0) for p, b in s.items()}} == dilated, (name, max_d2)
            for mode in D.MODES:
                assert equal(D.distance(pos, mrgb, mode, max_d2), D.distance_np(pos, mrgb, mode, max_d2)), (name, D.NAMES[mode], max_d2)
        flipped = mrgb.copy()
        flipped[:, 0] ^= 0x80                                              # bit 7 of the material byte never matters
        for mode in D.MODES:
            assert equal(D.distance_np(pos, mrgb, mode, 5), D.distance_np(pos, flipped, mode, 5)), name
            only, none, d2 = D.distance_np(pos, None, mode, 5)
            with_bytes = D.distance_np(pos, mrgb, mode, 5)
            assert none is None and np.array_equal(only, with_bytes[0]) and np.array_equal(d2, with_bytes[2])
        # against morphology, positions only: one step under the 6, 18 and 26 neighbourhoods is the ball of max_d2 1, 2 and 3
        for max_d2, c in ((1, 6), (2, 18), (3, 26)):
            assert np.array_equal(D.distance_np(pos, None, D.FIELD, max_d2)[0], M.morph(pos, None, M.MARGIN, c)[0]), (name, c)
            p, _, d2 = D.distance_np(pos, None, D.DEPTH, max_d2)
            assert np.array_equal(p[d2 <= max_d2], M.morph(pos, None, M.SURFACE, c)[0]), (name, c)
            assert np.array_equal(D.distance_np(pos, None, D.ERODE, max_d2)[0], M.morph(pos, None, M.ERODE, c)[0]), (name, c)
    assert len(T.source_of(*lists["random"])) < 500                   # it has duplicates, and the last entry's bytes win


RED, BLUE, GREEN = (1, 255, 0, 0), (2, 0, 0, 255), (3, 0, 255, 0)


def tie_cases():
    """[(pos, mrgb, max_d2, cell, the bytes it must take)]: a cell midway between two voxels takes the one at the negative offset,
    and at equal d2 the source is decided by dz before dy before dx."""
    cases = []
    for ax in range(3):
        for k in (1, 2, 5):
            lo, hi = [0, 0, 0], [0, 0, 0]
            lo[ax], hi[ax] = -k, k
            cases.append((np.array([hi, lo], np.int16), np.array([BLUE, RED], np.uint8), k * k, (0, 0, 0), RED))
    # d2 = 1 from three sides: (0, 0, +1) has rank(dz) = 2, the others rank(dz) = 0; of those (0, +1, 0) has rank(dy) = 2, (-1, 0, 0) has 0
    cases.append((np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.int16), np.array([RED, BLUE, GREEN], np.uint8), 1, (0, 0, 0), GREEN))
    cases.append((np.array([[0, 0, 1], [0, 1, 0]], np.int16), np.array([RED, BLUE], np.uint8), 1, (0, 0, 0), BLUE))
    cases.append((np.array([[0, 0, -1], [0, -1, 0], [-1, 0, 0]], np.int16), np.array([RED, BLUE, GREEN], np.uint8), 2, (0, 0, 0), GREEN))
    cases.append((np.array([[0, 0, -1], [0, -1, 0]], np.int16), np.array([RED, BLUE], np.uint8), 2, (0, 0, 0), BLUE))
    # d2 = 9 as (3, 0, 0) and as (-2, -2, -1): rank(dz) 0 against 1
    cases.append((np.array([[-2, -2, -1], [3, 0, 0]], np.int16), np.array([RED, BLUE], np.uint8), 9, (0, 0, 0), BLUE))
    cases.append((np.array([[2, 2, 0], [-2, 0, 2]], np.int16), np.array([RED, BLUE], np.uint8), 8, (0, 0, 0), RED))
    return cases


def test_the_ties():
    for pos, mrgb, max_d2, cell, want in tie_cases():
        for fn in (D.distance, D.distance_np):
            for order in ([0, 1, 2][:len(pos)], [2, 1, 0][-len(pos):]):
                for mode in (D.FIELD, D.DILATE):
                    got = as_dict(*fn(pos[order], mrgb[order], mode, max_d2))
                    assert got[cell][0] == want, (pos.tolist(), max_d2, got[cell])


# ---- the kernels' arithmetic as a host compiler reads it --------------------------------------------------------------------------
# The program takes cases "mode max_d2 m" + m lines "key word" and runs each as api_distance.hip and distance.hip do: the tiles of the
# list by their run heads, for FIELD and DILATE their windows sorted and the heads of that, then per candidate tile a block: the 54
# lower bounds, the occupancy rows, passes 1 and 2 plane by plane as the four waves deal them, pass 3 and the emission thread by
# thread, a new cell's source by the walk inside its tile's run.  Every array has exactly the kernel's size, so the sanitizer sees a
# read or write outside it.  It starts by printing ranks, offsets and radii.
DRIVER = r"""
#include <algorithm>
#include <cstdio>
#include <vector>
#include "distance_rule.h"
using namespace vxrt;

struct Out { uint64_t key; uint32_t word, d2; };

static int block(const std::vector<uint64_t>& keys, const std::vector<uint32_t>& words, uint64_t tile, uint32_t mode, uint32_t max_d2, std::vector<Out>* out) {
    const bool invert = mode == kDistanceDepth || mode == kDistanceErode;
    const uint32_t m = uint32_t(keys.size()), steps = distance_steps(m), last = m - 1u, R = distance_radius(max_d2), W = kDistanceTile + 2u * R;
    std::vector<uint64_t> rows(kDistanceRows, ~uint64_t(0)), run_tile(kDistanceWindowTiles);
    std::vector<uint16_t> slab(kDistanceSlab, 0x7777);
    std::vector<int8_t> slab_dy(kDistanceSlab, 99);
    std::vector<std::vector<int8_t>> plane(4, std::vector<int8_t>(kDistancePlane, 99));
    std::vector<uint32_t> run_lo(kDistanceWindowTiles), run_hi(kDistanceWindowTiles);
    for (uint32_t t = 0; t < kDistanceThreads; t++) {
        const uint32_t w = t < 2u * kDistanceWindowTiles ? t >> 1 : kDistanceWindowTiles - 1u;
        bool ok;
        const uint64_t nt = distance_window_tile(tile, w, &ok);
        const uint32_t found = distance_lower_bound(keys.data(), m, steps, (nt + (t & 1u)) << 12);
        if (found != uint32_t(std::lower_bound(keys.begin(), keys.end(), (nt + (t & 1u)) << 12) - keys.begin())) return 30;
        if (t < 2u * kDistanceWindowTiles) {
            if (t & 1u) run_hi[w] = ok ? found : 0u;
            else { run_lo[w] = ok ? found : 0u; run_tile[w] = nt; }
        }
    }
    for (uint32_t t = 0; t < kDistanceThreads; t++)
        for (uint32_t e = t; e < W * W; e += kDistanceThreads) rows[e] = 0u;
    for (uint32_t w = 0; w < kDistanceWindowTiles; w++) {
        const uint32_t lo = run_lo[w], hi = run_hi[w];
        if (hi < lo || hi - lo > 4096u) return 31;
        const int ox = (int(w / 9u) - 1) * 16 + int(R), oy = (int(w / 3u % 3u) - 1) * 16 + int(R), oz = (int(w % 3u) - 1) * 16 + int(R);
        for (uint32_t c = 0; c < kDistanceItems; c++) {
            if (uint64_t(lo) + c * kDistanceThreads >= hi) break;
            for (uint32_t t = 0; t < kDistanceThreads; t++) {
                const uint64_t i = uint64_t(lo) + c * kDistanceThreads + t;
                const uint64_t key = keys[i < last ? uint32_t(i) : last];
                uint32_t x, y, z;
                distance_cell_of(uint32_t(key) & 4095u, &x, &y, &z);
                if (distance_index_of(x, y, z) != (uint32_t(key) & 4095u)) return 32;
                const uint32_t wx = uint32_t(int(x) + ox), wy = uint32_t(int(y) + oy), wz = uint32_t(int(z) + oz);
                if (i < hi && wx < W && wy < W && wz < W) rows[wz * W + wy] |= uint64_t(1) << wx;
            }
        }
    }
    const uint64_t row_bits = (uint64_t(1) << W) - 1u;
    for (uint32_t it = 0; it < (W + 3u) / 4u; it++) {
        for (uint32_t wave = 0; wave < 4u; wave++) {
            const uint32_t wz = it * 4u + wave;
            if (wz >= W) continue;
            for (uint32_t lane = 0; lane < 64u; lane++)
                for (uint32_t k = 0; k < kDistancePlane / 64u; k++) {
                    const uint32_t e = k * 64u + lane, wy = e >> 4, x = e & 15u;
                    if (wy < W) {
                        const uint64_t row = (invert ? ~rows[wz * W + wy] : rows[wz * W + wy]) & row_bits;
                        plane[wave][e] = int8_t(distance_nearest(row, x + R, R));
                    }
                }
            for (uint32_t lane = 0; lane < 64u; lane++)
                for (uint32_t k = 0; k < 4u; k++) {
                    const uint32_t y = (lane >> 4) + 4u * k, x = lane & 15u;
                    uint32_t best = kDistanceFar;
                    int best_dy = 0;
                    for (uint32_t rank = 0; rank <= 2u * R; rank++) {
                        const int dy = distance_offset(rank);
                        if (distance_rank(dy) != rank) return 33;
                        distance_take_row(int(plane[wave][uint32_t(int(y + R) + dy) * 16u + x]), dy, &best, &best_dy);
                    }
                    slab[(wz * 16u + y) * 16u + x] = uint16_t(best);
                    if (!invert) slab_dy[(wz * 16u + y) * 16u + x] = int8_t(best_dy);
                }
        }
    }
    const bool bytes = !words.empty();
    uint32_t own = run_lo[13];
    for (uint32_t t = 0; t < kDistanceThreads; t++) {
        for (uint32_t j = 0; j < kDistanceItems; j++) {
            uint32_t x, y, z;
            distance_cell_of(t * kDistanceItems + j, &x, &y, &z);
            uint32_t best = kDistanceFar;
            int best_dz = 0;
            for (uint32_t rank = 0; rank <= 2u * R; rank++) {
                const int dz = distance_offset(rank);
                distance_take_plane(slab[(uint32_t(int(z + R) + dz) * 16u + y) * 16u + x], dz, &best, &best_dz);
            }
            const bool is_set = (rows[(z + R) * W + y + R] >> (x + R) & 1u) != 0u;
            const bool on = distance_emits(mode, is_set, best, max_d2);
            uint32_t word = 0;
            if (bytes) {
                uint32_t at;
                if (invert) {
                    at = own;
                    own += is_set ? 1u : 0u;
                } else {
                    const int dz = on ? best_dz : 0;
                    const uint32_t wz = uint32_t(int(z + R) + dz);
                    const int dy = on ? int(slab_dy[(wz * 16u + y) * 16u + x]) : 0;
                    const uint32_t wy = uint32_t(int(y + R) + dy);
                    const int step = distance_nearest(rows[wz * W + wy] & row_bits, x + R, R);
                    const int dx = on ? step : 0;
                    if (on && step == kDistanceNoStep) return 34;
                    const int sx = int(x) + dx, sy = int(y) + dy, sz = int(z) + dz;
                    const uint32_t w = on ? (sx < 0 ? 0u : sx < 16 ? 1u : 2u) * 9u + (sy < 0 ? 0u : sy < 16 ? 1u : 2u) * 3u + (sz < 0 ? 0u : sz < 16 ? 1u : 2u) : 13u;
                    const uint64_t q = run_tile[w] << 12 | distance_index_of(uint32_t(sx) & 15u, uint32_t(sy) & 15u, uint32_t(sz) & 15u);
                    at = distance_walk(keys.data(), last, run_lo[w], on ? run_hi[w] : run_lo[w], 12u, q);
                    if (on && keys[at] != q) return 35;
                    if (on && uint32_t(dx * dx + dy * dy + dz * dz) != best) return 36;
                }
                if (on && invert && keys[at] != (tile << 12 | (t * kDistanceItems + j))) return 37;
                word = words[at < last ? at : last];
            }
            if (on) out->push_back(Out{tile << 12 | (t * kDistanceItems + j), word, distance_value(best, max_d2)});
        }
    }
    return 0;
}

int main() {
    for (int d = -16; d <= 16; d++) std::printf("rank %d %u %d\n", d, distance_rank(d), distance_offset(distance_rank(d)));
    for (uint32_t v = 1; v <= kDistanceMaxD2; v++) std::printf("radius %u %u\n", v, distance_radius(v));
    unsigned mode, max_d2, m, with_words;
    while (std::scanf("%u %u %u %u", &mode, &max_d2, &with_words, &m) == 4) {
        std::vector<uint64_t> keys(m);
        std::vector<uint32_t> words(with_words ? m : 0);
        for (unsigned i = 0; i < m; i++) {
            unsigned long long k;
            unsigned w;
            if (std::scanf("%llu %u", &k, &w) != 2) return 2;
            keys[i] = k;
            if (with_words) words[i] = w;
        }
        std::vector<Out> out;
        if (m != 0) {
            const bool grow = mode == kDistanceField || mode == kDistanceDilate;
            std::vector<uint64_t> tiles;
            for (unsigned i = 0; i < m; i++) {
                if (i != 0 && keys[i] >> 12 == keys[i - 1] >> 12) continue;
                if (!grow) { tiles.push_back(keys[i] >> 12); continue; }
                for (uint32_t w = 0; w < kDistanceWindowTiles; w++) {
                    bool ok;
                    tiles.push_back(distance_window_tile(keys[i] >> 12, w, &ok));
                }
            }
            std::sort(tiles.begin(), tiles.end());
            tiles.erase(std::unique(tiles.begin(), tiles.end()), tiles.end());
            for (uint64_t tile : tiles)
                if (int rc = block(keys, words, tile, mode, max_d2, &out)) return rc;
        }
        for (const Out& e : out) std::printf("%llu %u %u\n", (unsigned long long)e.key, e.word, e.d2);
        std::printf("end %zu\n", out.size());
    }
    return 0;
}
"""


def tile_corner_voxels():
    """One voxel at each of the 8 positions u % 16 in {0, 15}^3 of a tile (u = p + 32768): its field spans 8 tiles."""
    return [np.array([[16 * 3 + a, -16 * 2 + b, 16 * 5 + c]], np.int16) for a in (0, 15) for b in (0, 15) for c in (0, 15)]


RANGE_CORNERS = np.array([[x, y, z] for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)], np.int16)


def key_cases():
    """[(pos, mrgb or None, [(mode, max_d2)])]"""
    rng = np.random.default_rng(31)
    colours = lambda n: rng.integers(0, 256, (n, 4)).astype(np.uint8)       # noqa: E731
    every = lambda *radii: [(mode, r) for mode in D.MODES for r in radii]     # noqa: E731
    cases = [(np.zeros((0, 3), np.int16), colours(0), every(1, 256))]
    for one in tile_corner_voxels():
        cases.append((one, colours(1), every(1, 3, 256)))
    cases.append((RANGE_CORNERS, colours(8), every(1, 3, 9, 256)))
    for pos, mrgb, max_d2, _, _ in tie_cases():
        cases.append((pos, mrgb, [(D.FIELD, max_d2), (D.DILATE, max_d2)]))
    cases.append((*M.cube16(), every(1, 3, 4, 49, 63, 64)))
    cases.append((*D.solid(31, -15), [(D.ERODE, 255), (D.ERODE, 256), (D.DEPTH, 256), (D.DILATE, 2)]))
    cases.append((*D.solid(33, -16), [(D.ERODE, 256), (D.DEPTH, 256), (D.FIELD, 3)]))
    for n in range(50):
        side = int(rng.choice([3, 6, 12, 20]))
        origin = np.array([int(rng.choice([-32768, -side // 2, 11, 32768 - side])) for _ in range(3)])
        count = int(rng.integers(1, 120))
        cells = (rng.integers(0, side, (count, 3)) + origin).astype(np.int16)
        max_d2 = int(rng.choice([1, 2, 3, 4, 9, 255, 256]))
        cases.append((cells, colours(count) if n % 5 else None, [(int(rng.choice(D.MODES)), max_d2), (int(rng.choice(D.MODES)), int(rng.choice([1, 2, 3, 4, 9])))]))
    return cases


def build_rule_program(tmp_path):
    src = tmp_path / "rule.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "rule"
    build = subprocess.run(SANITIZED + ["-I", CSRC, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return str(exe)


def run_rule_program(exe, runs):
    """runs: [(keys, words or None, mode, max_d2)] through the program -> [[(key, word, d2)]] per run, each held to the count the
    program prints behind it; the tables it prints first are held to the model's."""
    text = "".join(f"{mode} {max_d2} {0 if words is None else 1} {len(keys)}\n" + "".join(f"{k} {0 if words is None else words[i]}\n" for i, k in enumerate(keys))
                   for keys, words, mode, max_d2 in runs)
    run = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr.strip(), (run.returncode, run.stderr[-2000:])
    lines = iter(run.stdout.split("\n"))
    for d in range(-16, 17):
        assert next(lines) == f"rank {d} {D.rank(d)} {d}"
    for v in range(1, 257):
        assert next(lines) == f"radius {v} {D.radius(v)}"
    results = []
    for n, (keys, _, mode, max_d2) in enumerate(runs):
        got = []
        for line in lines:
            if line.startswith("end"):
                assert line == f"end {len(got)}", (n, D.NAMES[mode], max_d2, line, len(got))
                break
            got.append(tuple(int(v) for v in line.split()))
        results.append(got)
    assert next(lines) == ""
    return results


def model_keys(pos, mrgb, mode, max_d2):
    """What the program must print: [(path key, leaf word or 0, d2)] ascending."""
    out_pos, out_mrgb, d2 = D.distance_np(pos, mrgb, mode, max_d2)
    keys = D.path_keys_np(out_pos).tolist()
    words = [0] * len(keys) if out_mrgb is None else [M.leaf_word(b) for b in out_mrgb.tolist()]
    return list(zip(keys, words, d2.tolist()))


def test_the_kernels_arithmetic_under_the_sanitizers(tmp_path):
    exe = build_rule_program(tmp_path)
    runs, wants = [], []
    for pos, mrgb, params in key_cases():
        keys, words = M.sorted_keys_words(pos, mrgb)
        for mode, max_d2 in params:
            runs.append((keys, None if mrgb is None else words, mode, max_d2))
            wants.append(model_keys(pos, mrgb, mode, max_d2))
    kept_any = {mode: 0 for mode in D.MODES}
    for n, ((keys, words, mode, max_d2), got, want) in enumerate(zip(runs, run_rule_program(exe, runs), wants)):
        assert len(got) == len(want), (n, D.NAMES[mode], max_d2, len(keys), len(got), len(want))
        assert got == want, (n, D.NAMES[mode], max_d2, len(keys), next((g, w) for g, w in zip(got, want) if g != w))
        kept_any[mode] += len(want)
    assert all(kept_any.values())
