"""CPU: the device queries' interface (include/vxrt_query.h) — plain C, declared, exported with C linkage by both libraries, refused
without a context — the Python wrappers' signatures and argument checks, which run before any library call, and the lookup's model
(query_model.py) against something that does not follow its wording: a dense numpy grid of cube16 asked over every cell of the root
cube and a shell one cell wide outside it.  The oracle's bounded casts, which the GPU file relies on, are checked for the seven bounds."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

import query_model as Q
import ray_families as R
from conftest import ROOT
from test_components_cpu import bare_context, declared

FUNCTIONS = ["vxrt_lookup_voxels_device", "vxrt_pick_device"]
HEADER = "vxrt_query.h"
NEW_SOURCES = ("query.hip", "api_query.hip", "query.h")


def test_header_declares_exactly_the_two_entry_points():
    assert declared(HEADER) == FUNCTIONS
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other.endswith(".h") and other != HEADER:
            assert not set(FUNCTIONS) & set(declared(other)), other
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert '#include "vxrt.h"' in text and '#include "vxrt_edit.h"' in text
    assert "without wrap" in text and "byte for byte" in text and "vxrt_pick_hit" in text
    assert "typedef struct" not in text                                  # vxrt_pick_hit stays vxrt_edit.h's
    assert f'#include "{HEADER}"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        assert HEADER in open(os.path.join(ROOT, doc)).read(), doc
    assert "api_query.hip" in open(os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc", "ctx.h")).read()


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", HEADER)
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", "-I", os.path.join(ROOT, "include"), hdr],
                         capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text(f'#include "{HEADER}"\n'
                   '#include "vxrt_edit.h"\n'
                   'typedef char hit_is_36[sizeof(vxrt_pick_hit) == 36 ? 1 : -1];\n'
                   'int main(void) {\n'
                   '    size_t n = 7;\n'
                   '    const int32_t off[3] = {1, 0, 0};\n'
                   '    int a = vxrt_lookup_voxels_device(0, 0, 0, off, 0, &n);\n'
                   '    int b = vxrt_pick_device(0, 0, 0, 0, 0, 0);\n'
                   '    return a == VXRT_E_INVALID && b == VXRT_E_INVALID && n == 7 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)
    cpp = tmp_path / "c.cpp"
    cpp.write_text('#include "vxrt.hpp"\nstatic_assert(sizeof(vxrt_pick_hit) == 36, "vxrt_pick_hit");\n'
                   'size_t f(vxrt::Context& c, const int16_t (*p)[3], uint32_t* w) { return c.lookup_voxels_device(p, 1, {0, 0, 0}, w); }\n'
                   'void g(vxrt::Context& c, const float (*o)[3], const float* t, vxrt_pick_hit* h) { c.pick_device(o, o, t, 1, h); }\n')
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
    leaf = np.full(2, 0xABCD, np.uint32)
    rays = np.ones((2, 3), np.float32)
    bound = np.full(2, 4.0, np.float32)
    out = np.full(2 * 9, 0x5A5A5A5A, np.uint32)
    off = (C.c_int32 * 3)(1, 0, 0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = C.c_size_t(7)
    for count in (2, 0, 1 << 32):
        k = C.c_size_t(count)
        assert L.vxrt_lookup_voxels_device(None, p(pos), k, off, p(leaf), C.byref(n)) == H.E_INVALID
        assert L.vxrt_lookup_voxels_device(None, p(pos), k, None, None, C.byref(n)) == H.E_INVALID
        assert L.vxrt_lookup_voxels_device(None, None, k, None, None, None) == H.E_INVALID
        assert L.vxrt_pick_device(None, p(rays), p(rays), p(bound), k, p(out)) == H.E_INVALID
        assert L.vxrt_pick_device(None, p(rays), p(rays), None, k, p(out)) == H.E_INVALID
        assert L.vxrt_pick_device(None, None, None, None, k, None) == H.E_INVALID
    assert b"null context" in L.vxrt_last_error()
    assert n.value == 7 and (leaf == 0xABCD).all() and (out == 0x5A5A5A5A).all() and not pos.any()
    assert (rays == 1).all() and (bound == 4).all()


def test_the_new_sources_are_built_into_both_libraries():
    from gpu_voxel_raytracer_amd import _build
    csrc = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")
    for f in NEW_SOURCES:
        assert os.path.exists(os.path.join(csrc, f)), f
    assert "query.hip" in _build.SOURCES and "api_query.hip" in _build.SOURCES      # the variants build takes SOURCES too
    assert "query.h" in _build.HEADERS and any(h.endswith(HEADER) for h in _build.HEADERS)


def test_the_wrapper_has_the_three_methods(H):
    assert list(inspect.signature(H.Context.lookup_voxels).parameters) == ["self", "pos", "offset"]
    assert list(inspect.signature(H.Context.count_present).parameters) == ["self", "pos", "offset"]
    assert list(inspect.signature(H.Context.pick_device).parameters) == ["self", "origins", "dirs", "max_time"]
    for f in (H.Context.lookup_voxels, H.Context.count_present):
        assert inspect.signature(f).parameters["offset"].default is None
    assert inspect.signature(H.Context.pick_device).parameters["max_time"].default is None


def test_the_wrappers_check_their_arguments_before_any_library_call(H):
    import torch
    ctx = bare_context(H)
    try:
        pos = np.zeros((5, 3), np.int16)
        for method in (ctx.lookup_voxels, ctx.count_present):
            for bad in (pos.astype(np.int32), pos.astype(np.uint16), pos.astype(np.float32), torch.zeros((5, 3), dtype=torch.int32)):
                with pytest.raises(ValueError):
                    method(bad)                                           # dtype
            for bad in (np.zeros(15, np.int16), np.zeros((5, 4), np.int16), np.zeros((5, 3, 1), np.int16)):
                with pytest.raises(ValueError):
                    method(bad)                                           # not [n, 3]
            with pytest.raises(ValueError):
                method(torch.zeros((5, 3), dtype=torch.int16))            # a tensor of another device (the host's)
            for bad in (pos.tolist(), None, "pos"):
                with pytest.raises(TypeError):
                    method(bad)
            for bad in ((0, 0), (0, 0, 0, 0), (0.5, 0, 0), (2 ** 31, 0, 0), (0, -2 ** 31 - 1, 0), "abc", (None, 0, 0), 3):
                with pytest.raises(ValueError):
                    method(pos, bad)                                      # the offset, before pos is uploaded
        rays = np.ones((5, 3), np.float32)
        for bad in (rays.astype(np.float64), rays.astype(np.int32), torch.zeros((5, 3), dtype=torch.float64)):
            with pytest.raises(ValueError):
                ctx.pick_device(bad, rays)
            with pytest.raises(ValueError):
                ctx.pick_device(rays, bad)
        for bad in (np.ones(15, np.float32), np.ones((5, 4), np.float32)):
            with pytest.raises(ValueError):
                ctx.pick_device(bad, rays)
            with pytest.raises(ValueError):
                ctx.pick_device(rays, bad)
        with pytest.raises(ValueError):
            ctx.pick_device(torch.zeros((5, 3)), rays)                    # the host's tensor
        with pytest.raises(ValueError):
            ctx.pick_device(rays, np.ones((4, 3), np.float32))            # one direction per origin
        for bad in (rays.tolist(), None, "rays"):
            with pytest.raises(TypeError):
                ctx.pick_device(bad, rays)
            with pytest.raises(TypeError):
                ctx.pick_device(rays, bad)
        for bad in (np.ones(5, np.float64), np.ones((5, 1), np.float32), np.ones(4, np.float32), torch.ones(5)):
            with pytest.raises(ValueError):
                ctx.pick_device(rays, rays, bad)                          # max_time: dtype, shape, count, device
        for bad in ([1.0] * 5, "4.0", True):
            with pytest.raises(TypeError):
                ctx.pick_device(rays, rays, bad)
    finally:
        ctx._h = None                                                     # __del__ / close() have nothing to destroy


def test_a_tensor_that_is_not_contiguous_is_refused(H):
    import torch
    ctx = bare_context(H)
    try:
        with pytest.raises(ValueError, match="contiguous"):
            ctx.lookup_voxels(torch.zeros((3, 5), dtype=torch.int16).t())
        with pytest.raises(ValueError, match="contiguous"):
            ctx.pick_device(torch.zeros((3, 5)).t(), np.ones((5, 3), np.float32))
        with pytest.raises(ValueError, match="contiguous"):
            ctx.pick_device(np.ones((5, 3), np.float32), np.ones((5, 3), np.float32), torch.zeros(10)[::2])
    finally:
        ctx._h = None


# ---- the model against a dense grid ------------------------------------------------------------------------------------------------
def test_the_lookup_model_equals_a_dense_grid():
    pos, mrgb = R.scene_voxels("cube16")
    depth, half = 3, 8
    model = R.leaf_words(pos, mrgb)
    assert len(model) == len(pos)
    m = np.asarray(mrgb, np.uint32)
    words = np.uint32(0x80000000) | (m[:, 0] & 0x7F) << 24 | m[:, 1] << 16 | m[:, 2] << 8 | m[:, 3]
    # the root cube with a border of two cells, so that a shift by one never leaves the array
    pad = 2
    dense = np.zeros((2 * half + 2 * pad,) * 3, np.uint32)
    dense[tuple((pos.astype(np.int64) + half + pad).T)] = words
    assert np.count_nonzero(dense) == len(pos)
    g = np.arange(-half - 1, half + 1)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)     # the cube and its shell
    for offset in (None, (0, 0, 0), (1, 0, 0), (-16, 0, 0), (Q.INT32_MAX, 0, 0), (0, Q.INT32_MIN, 0)):
        got, present = Q.lookup(model, depth, cells, offset)
        off = np.zeros(3, np.int64) if offset is None else np.array(offset, np.int64)
        q = cells.astype(np.int64) + off
        inside = ((q >= -half) & (q < half)).all(1)
        want = np.zeros(len(cells), np.uint32)
        want[inside] = dense[tuple((q[inside] + half + pad).T)]
        assert np.array_equal(got.view(np.uint32), want), offset
        assert present == np.count_nonzero(want), offset
    assert Q.lookup(model, depth, cells, None)[1] == len(pos)
    shifted = Q.lookup(model, depth, cells, (-16, 0, 0))[0]
    at = np.flatnonzero(shifted)
    assert len(at) == int((pos[:, 0] == -half).sum()) and (cells[at, 0] == half).all()       # the shell's +x face sees the -x layer
    assert Q.lookup(model, depth, cells, (Q.INT32_MAX, 0, 0))[1] == 0
    # repeats count each time; an empty model and an empty list
    twice = np.concatenate([pos[:10], pos[:10], pos[:3]])
    assert Q.lookup(model, depth, twice)[1] == 23
    assert Q.lookup({}, 0, cells)[1] == 0 and Q.lookup(model, depth, np.zeros((0, 3), np.int16)) [1] == 0
    # a deeper root cube changes nothing but the range: the same voxels answer from outside the old cube's shell
    assert np.array_equal(Q.lookup(model, depth + 1, cells)[0], Q.lookup(model, depth, cells)[0])
    assert Q.lookup(model, 15, np.array([[32767, 3, -2]], np.int16), (1, 0, 0))[1] == 0


def test_the_oracle_casts_with_each_of_the_seven_bounds(O):
    """What the GPU file relies on: cast_rays takes every bound, a bound of 2^30 is the unbounded cast, a bounded hit is an unbounded
    hit no later than the bound allows, and the grouping of query_model.cast puts every ray's answer at the ray's index."""
    pos, mrgb = R.scene_voxels("cube16")
    octree = O.create_octree(pos, mrgb)
    root_half = R.root_half_of(octree)
    assert root_half == 4.0
    fam = R.scene_families("cube16", pos, root_half, n=700)
    model = R.leaf_words(pos, mrgb)
    words = set(model.values())
    for name, (o, d) in fam.items():
        free = Q.cast(O, octree, o, d)
        bounds = Q.dealt_bounds(len(o), root_half)
        assert [np.count_nonzero(np.arange(len(o)) % 7 == k) for k in range(7)] == [100] * 7
        got = Q.cast(O, octree, o, d, bounds)
        for k in range(7):
            at = np.flatnonzero(np.arange(len(o)) % 7 == k)
            b = float(bounds[at[0]])
            alone = O.cast_rays(octree, o[at], d[at], b)[:4]
            assert not R.differing_rays(tuple(x[at] for x in got), alone).any(), (name, Q.BOUNDS[k])
            if Q.BOUNDS[k] == "unbounded":
                assert not R.differing_rays(alone, tuple(x[at] for x in free)).any(), name
            hit = alone[0]
            assert set(alone[2][hit].tolist()) <= words | {-2 ** 31}, (name, Q.BOUNDS[k])
            if np.isfinite(b) and b < Q.UNBOUNDED:
                # a bounded cast never reports a hit the unbounded cast does not have
                assert not (hit & ~free[0][at]).any(), (name, Q.BOUNDS[k])
                same = hit & free[0][at]
                assert np.array_equal(alone[1][same].view(np.uint32), free[1][at][same].view(np.uint32)), (name, Q.BOUNDS[k])
        scalar = Q.cast(O, octree, o, d, 1.0)
        assert not R.differing_rays(scalar, O.cast_rays(octree, o, d, 1.0)[:4]).any()
    # the bounds do bound: with a bound of 0.25 fewer rays hit than without, in a family that starts outside the voxels
    o, d = fam["root_faces"]
    assert Q.cast(O, octree, o, d, 0.25)[0].sum() < Q.cast(O, octree, o, d)[0].sum()
