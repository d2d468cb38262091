"""CPU: the scene-depth extension's interface (include/vxrt_scene_depth.h) — plain C, declared, exported with C linkage, refused
without a device — the depth rule (host.scene_depth_for) against build_octree, and the model of the surgery (tests/scene_depth_model.py)
on host-built records at every depth from 0 to 15: the voxels stay and every block a node may widen in place is its own."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edit_model as M
import scene_depth_model as SD
from conftest import ROOT


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vxrt_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_exactly_the_two_entry_points():
    assert declared("vxrt_scene_depth.h") == ["vxrt_fit_scene_depth", "vxrt_set_scene_depth"]
    others = declared("vxrt.h") + declared("vxrt_edit.h") + declared("vxrt_grid_edit.h")
    assert "vxrt_set_scene_depth" not in others and "vxrt_fit_scene_depth" not in others
    assert '#include "vxrt.h"' in open(os.path.join(ROOT, "include", "vxrt_scene_depth.h")).read()
    assert '#include "vxrt_scene_depth.h"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "c.c"
    src.write_text('#include "vxrt_scene_depth.h"\n'
                   'int main(void) {\n'
                   '    uint32_t d = 0;\n'
                   '    int (*set)(vxrt_ctx*, uint32_t) = vxrt_set_scene_depth;\n'
                   '    int (*fit)(vxrt_ctx*, uint32_t*) = vxrt_fit_scene_depth;\n'
                   '    return set != 0 && fit != 0 && d == 0 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)


def test_library_exports_them_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    assert "vxrt_set_scene_depth" in exported and "vxrt_fit_scene_depth" in exported
    assert H.lib().vxrt_abi_version() == 6


def test_null_context_is_invalid_without_a_device(H):
    L = H.lib()
    d = C.c_uint32(77)
    assert L.vxrt_set_scene_depth(None, C.c_uint32(3)) == H.E_INVALID
    assert L.vxrt_set_scene_depth(None, C.c_uint32(16)) == H.E_INVALID
    assert L.vxrt_fit_scene_depth(None, C.byref(d)) == H.E_INVALID
    assert L.vxrt_fit_scene_depth(None, None) == H.E_INVALID
    assert d.value == 77


def rule_cases():
    rng = np.random.default_rng(3)
    cases = [np.zeros((0, 3), np.int16), np.array([[-1, -1, -1]]), np.array([[-4, -4, -4]]), np.array([[0, 0, 0]]),
             np.array([[-32768, 5, 5], [1, 2, 3]]), np.array([[32767, 0, 0]]), np.array([[-32768, -32768, -32767]]),
             np.array([[-32768, 0, 0], [32767, 32767, 32767]]), np.array([[-16384, -16384, -16384]]),
             np.array([[-4, -4, -4], [-4, -4, -3]]), np.array([[-4, -4, -4], [0, 0, 0]])]
    for k in range(16):
        lim = 1 << k
        cases.append(rng.integers(-lim, lim, size=(int(rng.integers(1, 40)), 3)))
        cases.append(rng.integers(max(-lim, -32768), min(lim, 32768), size=(3, 3)) // 2)
        cases.append(np.array([[-lim, -lim, -lim]]) if lim < 32768 else np.array([[-32767, 0, 0]]))
    return [np.asarray(c, np.int16).reshape(-1, 3) for c in cases]


def test_the_depth_rule_equals_build_octree(H):
    for pos in rule_cases():
        want = H.build_octree(pos, np.full((len(pos), 4), 9, np.uint8))[1]
        assert H.scene_depth_for(pos) == want, pos.tolist()
    with pytest.raises(H.VxrtError):        # the one case whose rule gives 16: every build refuses it
        H.build_octree(np.array([[-32768] * 3], np.int16), np.full((1, 4), 9, np.uint8))
    assert H.scene_depth_for([[-32768] * 3]) == 16
    assert H.scene_depth_for([[-1, -1, -1]]) == 1 and H.scene_depth_for([[-4, -4, -4]]) == 3


def unique(pos):
    return np.unique(np.asarray(pos, np.int16).reshape(-1, 3), axis=0)


def test_the_model_fit_equals_the_rule(H):
    for pos in rule_cases():
        pos = unique(pos)
        mrgb = np.full((len(pos), 4), 9, np.uint8)
        s = SD.Scene.build(H, pos, mrgb)
        want = H.build_octree(pos, mrgb)[1]
        SD.set_depth(s, 15)                  # from the top: the fit shrinks (or, for (-2^k)^3, lands one above the least cube)
        assert SD.fit(s) == want, pos.tolist()
        assert M.decode_records(*s.arrays(), s.depth) == M.from_list(pos, mrgb)
        assert s.live == len(H.build_records(pos, mrgb)[0])
        SD.set_depth(s, 15)
        SD.set_depth(s, want)
        assert s.live == len(H.build_records(pos, mrgb)[0])
    one = SD.Scene.build(H, np.array([[-16384] * 3], np.int16), np.full((1, 4), 9, np.uint8))
    assert one.depth == 15
    SD.set_depth(one, 14)                    # its least cube
    with pytest.raises(SD.Refused):
        SD.set_depth(one, 13)
    assert SD.fit(one) == 15


def scene_lists(H, scenes):
    rng = np.random.default_rng(8)
    pos, mrgb, _ = scenes.load_scene("castle")
    yield "castle", pos, mrgb
    pos = unique(rng.integers(-8, 8, size=(300, 3)))
    yield "random", pos, rng.integers(0, 256, size=(len(pos), 4)).astype(np.uint8)
    yield "one voxel", np.array([[-1, -1, -1]], np.int16), np.array([[1, 2, 3, 4]], np.uint8)
    yield "empty", np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)


def test_model_surgery_keeps_the_voxels_and_the_storage_rule_at_every_depth(H, scenes):
    for name, pos, mrgb in scene_lists(H, scenes):
        want = M.from_list(pos, mrgb)
        s = SD.Scene.build(H, pos, mrgb)
        d0 = s.depth
        # up one level at a time, then down one at a time, then jumps both ways
        path = list(range(d0 + 1, 16)) + list(range(14, -1, -1)) + [15, d0, 9, 15, 0, 15]
        least = H.cube_depth(pos.min(0), pos.max(0)) if len(pos) else 0
        for d in path:
            try:
                SD.set_depth(s, d)
            except SD.Refused:
                assert d < least, (name, d)
                continue
            assert d >= least and s.depth == d
            assert M.decode_records(*s.arrays(), d) == want, (name, d)
            assert SD.block_owners(s), (name, d)
        assert SD.fit(s) == H.scene_depth_for(pos)
        assert M.decode_records(*s.arrays(), s.depth) == want


def test_model_refuses_a_shrink_that_would_drop_a_voxel(H):
    pos = np.array([[0, 0, 0], [7, -8, 3]], np.int16)
    mrgb = np.full((2, 4), 5, np.uint8)
    s = SD.Scene.build(H, pos, mrgb)
    assert s.depth == 3
    SD.set_depth(s, 15)
    SD.set_depth(s, 3)
    before = s.arrays()
    with pytest.raises(SD.Refused):
        SD.set_depth(s, 2)
    after = s.arrays()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and s.depth == 3


def test_grown_blocks_are_not_shared_after_edits(H):
    """The storage rule's pitfall, in the model: a scene whose root block an edit allocated (so at or beyond the build counts) grows;
    every new node has a block of its own, so a later widening in place cannot run over a sibling."""
    pos = np.array([[0, 0, 0], [-3, 2, 1], [1, -2, -1]], np.int16)
    mrgb = np.full((3, 4), 5, np.uint8)
    svo, _, leaves, depth = H.build_records(pos, mrgb)
    s = SD.Scene(svo, leaves, depth)
    # what an edit that moved the root's children to an 8-entry block leaves: the old block a hole, the new one at the end
    M_ = s.svo[0][0] & 0xFF
    n = bin(M_).count("1")
    s.built = (len(s.svo), len(s.leaves))
    moved = [list(s.svo[s.svo[0][1] + i]) for i in range(n)] + [[0, 0]] * (8 - n)
    s.svo[0] = [M_, len(s.svo)]
    s.svo += moved
    assert SD.block_owners(s)
    SD.set_depth(s, depth + 1)
    assert SD.block_owners(s)
    assert M.decode_records(*s.arrays(), s.depth) == M.from_list(pos, mrgb)
    base = s.svo[0][1]
    for r in range(n):
        node = s.svo[base + r]
        assert bin(node[0] & 0xFF).count("1") == 1 and node[1] >= s.built[0] and node[1] != s.svo[base + (r + 1) % n][1]
