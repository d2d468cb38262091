"""CPU: the compaction extension's interface (include/vxrt_compact.h) — plain C, declared once, exported with C linkage by both
libraries, refused without a context — and the model of the relayout (tests/compact_model.py) against the host builder
(vxrt_build_records): whatever the layout of a tree's records, the model returns the bytes a fresh build has."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import compact_model as CM
import edit_model as M
import scene_depth_model as SD
from conftest import ROOT


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vxrt_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_exactly_the_two_entry_points():
    assert declared("vxrt_compact.h") == ["vxrt_compact_scene", "vxrt_get_scene_storage"]
    others = sum((declared(h) for h in os.listdir(os.path.join(ROOT, "include")) if h.endswith(".h") and h != "vxrt_compact.h"), [])
    assert "vxrt_compact_scene" not in others and "vxrt_get_scene_storage" not in others
    assert '#include "vxrt.h"' in open(os.path.join(ROOT, "include", "vxrt_compact.h")).read()
    assert '#include "vxrt_compact.h"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()


def test_header_is_plain_c(tmp_path):
    hdr = os.path.join(ROOT, "include", "vxrt_compact.h")
    chk = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-pedantic", "-fsyntax-only", "-x", "c", hdr], capture_output=True, text=True)
    assert chk.returncode == 0 and not chk.stderr.strip(), chk.stderr
    src = tmp_path / "c.c"
    src.write_text('#include "vxrt_compact.h"\n'
                   'int main(void) {\n'
                   '    vxrt_scene_storage s;\n'
                   '    int (*compact)(vxrt_ctx*) = vxrt_compact_scene;\n'
                   '    int (*storage)(vxrt_ctx*, vxrt_scene_storage*) = vxrt_get_scene_storage;\n'
                   '    s.records_live = s.records_used = s.records_capacity = s.leaves_used = s.leaves_capacity = 0;\n'
                   '    return compact != 0 && storage != 0 && sizeof s == 40 && s.records_live == 0 ? 0 : 1;\n'
                   '}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "c.o")], check=True)


def test_both_libraries_export_them_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    for path in (_build.LIB, H.variants_library()):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
        exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
        assert "vxrt_compact_scene" in exported and "vxrt_get_scene_storage" in exported, path
    assert H.lib().vxrt_abi_version() == 6
    assert C.sizeof(H.SceneStorage) == 40
    assert callable(H.Context.compact_scene) and callable(H.Context.scene_storage)


def test_null_arguments_are_invalid_without_a_device(H):
    L = H.lib()
    s = H.SceneStorage(7, 7, 7, 7, 7)
    assert L.vxrt_compact_scene(None) == H.E_INVALID
    assert L.vxrt_get_scene_storage(None, C.byref(s)) == H.E_INVALID
    assert L.vxrt_get_scene_storage(None, None) == H.E_INVALID
    assert [getattr(s, n) for n, _ in H.SceneStorage._fields_] == [7] * 5


def unique(pos):
    return np.unique(np.asarray(pos, np.int16).reshape(-1, 3), axis=0)


def scene_lists(H, scenes):
    rng = np.random.default_rng(21)
    for name in ("menger", "castle", "8x8x8", "chr_knight"):
        pos, mrgb, _ = scenes.load_scene(name)
        yield name, pos, mrgb
    pos, mrgb = H.default_scene_voxels(1)
    yield "startup", pos, mrgb
    pos = unique(rng.integers(-16, 16, size=(500, 3)))
    yield "random", pos, rng.integers(0, 256, size=(len(pos), 4)).astype(np.uint8)
    yield "empty", np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    yield "one voxel", np.array([[-1, -1, -1]], np.int16), np.array([[1, 2, 3, 4]], np.uint8)
    yield "depth 0", np.array([[0, 0, 0], [-1, 0, -1], [0, -1, 0]], np.int16), np.array([[1, 2, 3, 4], [0, 9, 8, 7], [2, 5, 5, 5]], np.uint8)


def built(H, pos, mrgb):
    """The builder's bytes as the device holds them (api_scene.hip: upload_svo keeps one leaf word for an empty list)."""
    svo, _, leaves, depth = H.build_records(pos, mrgb)
    if len(leaves) == 0:
        leaves = np.zeros(1, np.int32)
    return svo, leaves, depth


def same(got, want):
    return (got[0].dtype == np.uint32 and got[1].dtype == np.int32 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
            and np.array_equal(got[1], want[1]))


def test_the_model_keeps_the_builders_bytes(H, scenes):
    for name, pos, mrgb in scene_lists(H, scenes):
        svo, leaves, depth = built(H, pos, mrgb)
        assert same(CM.compact(svo, leaves, depth), (svo, leaves)), name
    assert built(H, np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8))[0].tolist() == [[0, 1]]
    assert built(H, *list(scene_lists(H, scenes))[-1][1:])[2] == 0


def test_the_model_restores_the_builders_bytes_from_any_layout(H, scenes):
    rng = np.random.default_rng(34)
    for name, pos, mrgb in scene_lists(H, scenes):
        svo, leaves, depth = built(H, pos, mrgb)
        want = (svo, leaves)
        # sibling blocks in a random order with slack between them
        moved = CM.damage(svo, leaves, depth, rng)
        if len(pos) > 100:
            assert len(moved[0]) > len(svo) or len(moved[1]) > len(leaves), name
        assert M.decode_records(*moved, depth) == M.from_list(pos, mrgb), name
        assert same(CM.compact(*moved, depth), want), name
        # what depth changes leave: holes and 8-entry blocks (scene_depth_model), then the same permutation on top
        s = SD.Scene(svo, leaves, depth)
        for up in sorted({min(depth + 1, 15), min(depth + 3, 15), 15}):
            if up == depth:
                continue
            SD.set_depth(s, up)
            grown = s.arrays()
            at_depth = CM.compact(*grown, up)           # the undamaged arrays at that depth
            assert M.decode_records(*at_depth, up) == M.from_list(pos, mrgb), (name, up)
            assert same(CM.compact(*CM.damage(*grown, up, rng), up), at_depth), (name, up)
            if len(pos):
                assert len(at_depth[0]) == s.live and len(at_depth[0]) < len(grown[0]), (name, up)
            SD.set_depth(s, depth)
            back = s.arrays()
            if len(pos):
                assert len(back[0]) > len(svo), name          # the shrink left the grown blocks behind as holes
            assert same(CM.compact(*back, depth), want), (name, up)
            assert same(CM.compact(*CM.damage(*back, depth, rng), depth), want), (name, up)
        if len(pos) > 1:
            assert SD.fit(s) == depth
            assert same(CM.compact(*s.arrays(), depth), want), name


def test_the_model_is_idempotent_and_reads_no_unreachable_entry(H, scenes):
    rng = np.random.default_rng(5)
    pos, mrgb, _ = scenes.load_scene("castle")
    svo, leaves, depth = built(H, pos, mrgb)
    a = CM.damage(svo, leaves, depth, rng, slack=5)
    b = CM.damage(svo, leaves, depth, rng, slack=0)     # other junk, other order
    once = CM.compact(*a, depth)
    assert same(once, CM.compact(*b, depth))
    assert same(CM.compact(*once, depth), once)
    with pytest.raises(AssertionError):
        CM.compact(np.array([[1, 1], [0, 0]], np.uint32), np.zeros(1, np.int32), 1)   # a leaf parent without a leaf word
