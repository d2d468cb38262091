"""CPU: the device-build extension's interface (include/vxrt_device_scene.h) — declared, exported with C linkage, refused without a
device where it must be — and the Python model (tests/device_build_model.py) of the layout the device builds, checked against the
host builder (vxrt_build_records) on every fixture and on random, extreme, deep and empty lists."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import device_build_model as D
from conftest import ROOT, reference_vox, reference_vox_names


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(vxrt_[a-z_0-9]+)\s*\(", text)))


def test_header_declares_exactly_set_voxels_device():
    assert declared("vxrt_device_scene.h") == ["vxrt_set_voxels_device"]
    assert '#include "vxrt.h"' in open(os.path.join(ROOT, "include", "vxrt_device_scene.h")).read()
    assert len(declared("vxrt.h")) <= 40
    assert "vxrt_device_scene.h" in open(os.path.join(ROOT, "include", "vxrt.h")).read()
    assert '#include "vxrt_device_scene.h"' in open(os.path.join(ROOT, "include", "vxrt.hpp")).read()


def test_library_exports_set_voxels_device_with_c_linkage(H):
    from gpu_voxel_raytracer_amd import _build
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], capture_output=True, text=True).stdout
    exported = [l.split()[-1] for l in out.splitlines() if " T " in l]
    assert "vxrt_set_voxels_device" in exported
    assert H.lib().vxrt_abi_version() == 6


def test_refusals_without_a_device(H):
    L = H.lib()
    pos = np.zeros((1, 3), np.int16)
    mrgb = np.zeros((1, 4), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert L.vxrt_set_voxels_device(None, p(pos), p(mrgb), C.c_size_t(1)) == H.E_INVALID
    assert L.vxrt_set_voxels_device(None, None, None, C.c_size_t(0)) == H.E_INVALID


def assert_same_records(H, pos, mrgb, what=""):
    svo, _, leaves, depth = H.build_records(pos, mrgb)
    msvo, mleaves, mdepth = D.build(pos, mrgb)
    assert mdepth == depth, what
    assert np.array_equal(msvo, svo), f"{what}: records"
    assert np.array_equal(mleaves, leaves), f"{what}: leaf words"
    assert D.record_count(pos) == len(svo), what


@pytest.mark.parametrize("name", reference_vox_names())
def test_model_equals_host_builder_on_fixtures(H, name):
    pos, mrgb, _ = H.vox_to_voxels(reference_vox(name))
    assert_same_records(H, pos, mrgb, name)


def random_list(rng, n, lim, dup):
    pos = rng.integers(-lim, lim, (n, 3)).astype(np.int16)
    if dup:
        pos = np.concatenate([pos, pos[rng.integers(0, n, n // 2)]])
    mrgb = rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)
    order = rng.permutation(len(pos))
    return pos[order], mrgb[order]


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_host_builder_on_random_lists(H, seed):
    rng = np.random.default_rng(seed)
    lim = [1, 3, 17, 200, 5000, 32768][seed]
    pos, mrgb = random_list(rng, 3000, lim, dup=seed % 2 == 0)
    assert_same_records(H, pos, mrgb, f"seed {seed}")
    # duplicates: the last entry wins, whichever order they come in
    assert_same_records(H, pos[::-1], mrgb[::-1], f"seed {seed} reversed")


def test_model_equals_host_builder_on_extremes(H):
    e = np.array([-32768, 32767, 0, -1], np.int16)
    pos = np.stack(np.meshgrid(e, e, e, indexing="ij"), axis=-1).reshape(-1, 3)
    mrgb = (np.arange(len(pos) * 4) % 251).astype(np.uint8).reshape(-1, 4)
    assert_same_records(H, pos, mrgb, "extremes")


@pytest.mark.parametrize("depth", range(16))
def test_model_equals_host_builder_one_voxel_at_every_depth(H, depth):
    pos = np.array([[(1 << depth) - 1, 0, 0]], np.int16)
    mrgb = np.array([[0xC5, 1, 2, 3]], np.uint8)
    assert D.depth_of(pos) == depth
    assert_same_records(H, pos, mrgb, f"depth {depth}")


def test_model_equals_host_builder_on_the_empty_list(H):
    assert_same_records(H, np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8), "empty")


def test_depth_rule_refuses_what_the_host_refuses(H):
    pos = np.full((2, 3), -32768, np.int16)        # max = -32768: |max| + 1 = 32769 -> depth 16
    assert D.depth_of(pos) is None
    with pytest.raises(H.VxrtError) as e:
        H.build_records(pos, np.zeros((2, 4), np.uint8))
    assert e.value.status == H.E_SCENE
