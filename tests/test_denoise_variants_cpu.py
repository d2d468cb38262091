"""CPU: every denoise kernel launch_denoise can pick has a parity case.  The pair kernel is compiled once per radius (csrc/post.hip:
VXRT_PAIR); tests/test_gpu_denoise.py sweeps a radius list of its own.  A radius added to one and not the others fails here."""
import os
import re

import numpy as np

import test_gpu_denoise as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpu_voxel_raytracer_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_every_compiled_denoise_radius_has_a_parity_case():
    lines = [ln for ln in _read("post.hip").splitlines() if ln.strip().startswith("VXRT_PAIR(")]
    assert len(lines) == 1, lines
    compiled = tuple(int(r) for r in re.findall(r"VXRT_PAIR\((\d+)\)", lines[0]))
    bound = re.findall(r"d->radius > (\d+)\)", _read("api_context.hip"))
    assert len(bound) == 1, bound
    n = int(bound[0])
    assert compiled == tuple(range(1, n + 1)), (compiled, n)
    assert T.PAIR_RADII == compiled
    assert T.SWEEP_RADII == (0,) + compiled
    assert tuple(sorted(T.BAND_LAYOUTS)) == compiled


def test_sweep_frames_hold_both_block_kinds():
    """The planned G-buffers of the GPU sweep: exotic exactly where planned, and lean and careful blocks side by side at every radius."""
    for (w, h), at in T.SWEEP_FRAMES.items():
        color, nd, _ = T.planned_gbuffer(w, h, seed=w * 1000 + h, exotic_at=at)
        exotic = T.exotic_pixels(color, nd)
        assert sorted(map(tuple, np.argwhere(exotic))) == sorted(set(at))
        for r in T.PAIR_RADII:
            T.assert_both_paths(exotic, r, f"{w}x{h}, radius {r}")


def test_careful_blocks_geometry():
    exotic = np.zeros((40, 70), bool)
    exotic[20, 40] = True                                    # tile (1, 1) of 32x16
    assert T.careful_blocks(exotic, 1).tolist() == [[False, False, False], [False, True, False], [False, False, False]]
    assert T.careful_blocks(exotic, 4).tolist() == [[False, False, False], [False, True, False], [False, False, False]]
    assert T.careful_blocks(exotic, 5).tolist() == [[False, True, False], [False, True, False], [False, False, False]]
    exotic[:] = False
    exotic[24, 39] = True                                    # the apron of tile (t, c) is rows 16 t - r .. 16 t + 15 + r
    assert T.careful_blocks(exotic, 8).tolist() == [[False, False, False], [True, True, False], [True, True, False]]
    exotic[:] = False
    exotic[0, 69] = True
    rows = np.r_[16:32]                                      # a rank that holds frame rows 16 .. 31 only
    assert T.careful_blocks(exotic, 8, rows).tolist() == [[False, False, False]]
    rows = np.r_[8:24]
    assert T.careful_blocks(exotic, 8, rows).tolist() == [[False, True, True]]   # columns 24 .. 71 and 56 .. 103


def test_fast_sigma_range_edge():
    lo, hi = T.fast_sigma_range_edge()
    assert lo.dtype == np.float32 and hi == np.nextafter(lo, np.float32(np.inf))
    assert 7.07 < lo < hi < 7.072
