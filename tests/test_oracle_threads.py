"""CPU: the oracle's default thread count follows the CPUs this process may use, and its results do not depend on the count."""
import os

import numpy as np


def test_default_threads_is_capped(O, monkeypatch):
    mine = len(os.sched_getaffinity(0))
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    assert O.default_threads() == mine
    monkeypatch.setenv("OMP_NUM_THREADS", "1")
    assert O.default_threads() == 1
    monkeypatch.setenv("OMP_NUM_THREADS", str(mine + 100))
    assert O.default_threads() == mine
    monkeypatch.setenv("OMP_NUM_THREADS", "")
    assert O.default_threads() == mine


def test_denoise_and_trace_do_not_depend_on_the_thread_count(O, scenes, noise, monkeypatch):
    monkeypatch.delenv("OMP_NUM_THREADS", raising=False)
    w, h = 64, 40
    pos, mrgb, size = scenes.load_scene("castle")
    cam = scenes.close_camera(size)
    u = O.Uniforms.default()
    u.set_camera(cam[0], O.camera_axis_scaled(cam[0], cam[1], cam[2], w, h))
    u.frame_number = 3
    octree = O.create_octree(pos, mrgb)
    one = O.trace(octree, noise, u, w, h, 3, crop=(0, 0, w, h), nthreads=1)
    default = O.trace(octree, noise, u, w, h, 3, crop=(0, 0, w, h))
    for a, b in zip(one[:3], default[:3]):
        assert a.tobytes() == b.tobytes()
    assert one[3] == default[3]
    du = O.Denoise.default()
    du.radius = 5
    color, nd, alb = one[:3]
    d1 = O.denoise(color, nd, alb, u.camera16(), du, nthreads=1)
    dd = O.denoise(color, nd, alb, u.camera16(), du)
    assert d1.tobytes() == dd.tobytes() and np.isfinite(d1).mean() > 0.5
