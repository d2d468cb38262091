"""GPU: a context that has been through every path that replaces or re-allocates what it holds (a second scene, an edit that grows
the storage, a compaction, a change of depth, a tail-capacity change, two resizes, the scene set again) renders the same frames,
bit for bit, and holds the same device records as a fresh context."""
import numpy as np
import pytest

from conftest import assert_bits_equal

pytestmark = pytest.mark.gpu

W, H_ = 64, 48
IMAGES = ("SAMPLED_COLOR", "NORMAL_DEPTH", "ALBEDO_NODE", "ACCUM_COLOR", "DENOISED")


def two_frames(H, ctx, scene):
    """The scene set, then frames 100 and 101 from a fixed camera -> every image of the second, and the device records."""
    ctx.recreate_octree(*scene)
    ctx.camera = H.Camera()
    ctx.reset_history()
    ctx.set_frame_number(100)
    ctx.render_frames(H.ALL, 2)
    ctx.sync()
    return {name: ctx.read(getattr(H, name)) for name in IMAGES}, ctx.read_scene()


def test_a_context_after_every_replacement_equals_a_fresh_one(H):
    scene = H.default_scene_voxels()
    with H.Context(W, H_, frames_per_launch=2) as used:
        used.recreate_octree(*scene)
        used.render_frames(H.ALL, 2)
        depth = used.scene_depth
        before = used.scene_storage()
        used.edit_voxels(np.array([[1, 2, 3], [-4, 5, -6]], np.int16), [[1, 200, 30, 30], [2, 30, 200, 30]])   # tight storage: any set grows it
        assert used.scene_storage()["records_capacity"] > before["records_capacity"]
        used.compact_scene()
        used.set_scene_depth(depth + 2)
        used.render_frames(H.ALL, 2)
        used.set_option(H.OPT_TAIL_CAPACITY, 128)
        used.set_option(H.OPT_TAIL_CAPACITY, 0)
        used.resize(80, 32)
        used.render_frames(H.ALL, 2)
        used.resize(W, H_)
        got, got_scene = two_frames(H, used, scene)
    with H.Context(W, H_, frames_per_launch=2) as fresh:
        want, want_scene = two_frames(H, fresh, scene)
    for name in IMAGES:
        assert_bits_equal(got[name], want[name], name)
    assert np.isfinite(want["DENOISED"]).all() and want["SAMPLED_COLOR"].any()
    for a, b in zip(got_scene, want_scene):
        assert np.array_equal(a, b)
