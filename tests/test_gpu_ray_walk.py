"""GPU: the octree walk (cast_ray, csrc/trace_common.h) ray by ray against the oracle's cast_bounded_ray on the ray families of
tests/ray_families.py — origins on node planes and on the root's faces, signed-zero / subnormal / huge direction components, origins
1e30 away, non-finite origins and directions — through every walk (vxrt_debug_cast_rays and vxrt_pick; 8-byte and wide records;
treelet node orders), every way a tree gets into device memory, and frames from cameras the walk dislikes.
Bar: bit-exact — hit flag, time bits (the time of a miss too), leaf word, normal bits with the signs of zero — with ONE pinned
difference, the sign of a zero time (check_walks).  Measured on an MI355X, rays of that class per 20 000: cube16 on_planes 31,
cube32 on_planes 19, one_voxel root_faces 201 (each run prints its own counts).  Before walkf_begin took the root test's max / min in
the shader's operand order, 37 of the 64 cases here failed: every scene's nonfinite_origin family (origin.x = NaN: 1 177 of 20 000 rays
on castle, 672 on the empty scene, 1 255 on deep15) and every frame from the camera at (NaN, 1, -9)."""
import numpy as np
import pytest
# torch's HIP runtime must be the process's first (set_voxels_device below): imported at collection, as tests/test_gpu_device_build.py does
import torch  # noqa: F401

import ray_families as R
from conftest import assert_bits_equal, require_variants

pytestmark = pytest.mark.gpu

_REF = {}


def reference(O, key, pos, mrgb, aim=None):
    """The oracle's side of one voxel set, computed once and shared: octree, voxel model, the families and what the oracle casts.
    aim: the voxels the families are aimed at (default: all of them)."""
    if key not in _REF:
        name = key if key in R.SCENES else key.split("+")[0]
        octree = O.create_octree(pos, mrgb)
        fam = R.scene_families(name, pos if aim is None else aim, R.root_half_of(octree))
        want = {k: O.cast_rays(octree, o, d)[:4] for k, (o, d) in fam.items()}
        model = R.leaf_words(pos, mrgb)
        keys = _voxel_keys(np.array(sorted(model), np.int64).reshape(-1, 3))     # ascending, as the tuples are
        words = np.array([model[p] for p in sorted(model)], np.int32)
        assert (np.diff(keys) > 0).all()
        _REF[key] = dict(pos=pos, mrgb=mrgb, octree=octree, depth=O.voxel_depth(pos), fam=fam, want=want, keys=keys, words=words)
    return _REF[key]


def _voxel_keys(v):
    v = np.asarray(v, np.int64).reshape(-1, 3) + 32768
    return v[:, 0] << 32 | v[:, 1] << 16 | v[:, 2]


def scene_reference(O, scenes, name):
    return reference(O, name, *R.scene_voxels(name, scenes))


def check_walks(ctx, ref, what, only=None):
    """vxrt_debug_cast_rays and vxrt_pick against the oracle, family by family -> {family: rays of the pinned difference}.

    The pinned difference (the sign of a zero time; csrc/trace_common.h above WalkF): a ray may differ from the
    oracle in the sign bit of a zero `time` — device -0, oracle +0 — and in nothing else, and only if its origin has a coordinate
    exactly on a multiple of the finest cell.  Every other difference fails.  Both probes must show it on the same rays."""
    pinned = {}
    for family, (o, d) in ref["fam"].items():
        if only is not None and family not in only:
            continue
        want = ref["want"][family]
        got = ctx.cast_rays(o, d)
        pinned[family] = R.assert_rays_equal(got, want, f"{what}: cast_rays, {family}", o, d, zero_time_sign=True)
        p = ctx.pick(o, d)
        assert np.isin(p["status"], (0, 1, 2)).all()
        picked = (p["status"] != 0, p["time"], p["leaf"], p["normal"])
        R.assert_rays_equal(picked, got, f"{what}: pick against cast_rays, {family}", o, d)           # the two probes: bit for bit
        assert R.assert_rays_equal(picked, want, f"{what}: pick, {family}", o, d, zero_time_sign=True) == pinned[family]
        assert np.array_equal(p["status"] == 2, p["leaf"] == np.int32(-2 ** 31)), f"{what}: pick, {family}: status 2 <=> the cap's leaf word"
        # status 1: the voxel is in the voxel model with that leaf word (independent of the tree)
        hit = p["status"] == 1
        k = _voxel_keys(p["voxel"][hit])
        at = np.searchsorted(ref["keys"], k)
        at = np.minimum(at, max(len(ref["keys"]) - 1, 0))
        assert not hit.any() or (np.array_equal(ref["keys"][at], k) and np.array_equal(ref["words"][at], p["leaf"][hit])), \
            f"{what}: pick, {family}: a picked voxel is not in the model with its leaf word"
        assert (p["voxel"][~hit] == 0).all()
    print(f"{what}: rays that differ in the sign of a zero time only: {pinned}")
    return pinned


WALKS = [(scene, mode) for scene in R.SCENES for mode in ("records8", "wide")] + \
        [(scene, mode) for scene in ("cube32", "castle", "deep15") for mode in ("order2", "order3")]     # treelets need depth >= 4


@pytest.mark.parametrize("scene,mode", WALKS)
def test_every_walk_equals_the_oracle_on_every_family(O, H, scenes, monkeypatch, scene, mode):
    """(a) 20 000 rays per family and scene through both probes: the 8-byte records, the wide records (VXRT_WIDE=1), and the last two /
    three node levels laid out as treelets (VXRT_OPT_NODE_ORDER 2 / 3)."""
    ref = scene_reference(O, scenes, scene)
    tuning = []
    if mode == "wide":
        require_variants(H, wide="1")
        monkeypatch.setenv("VXRT_WIDE", "1")
    elif mode != "records8":
        tuning = [(H.OPT_NODE_ORDER, int(mode[-1]))]
    with H.Context(32, 32, tuning=tuning) as ctx:
        ctx.recreate_octree(ref["pos"], ref["mrgb"])
        st = ctx.stats()
        assert st.octree_depth == ref["depth"]
        assert st.scene_format == (1 if mode == "wide" else 0)
        assert st.node_order == (int(mode[-1]) if mode.startswith("order") else 0)
        check_walks(ctx, ref, f"{scene} {mode}")


STATE_FAMILIES = ("on_planes", "root_faces", "zero_components", "nonfinite_origin")


@pytest.mark.parametrize("state", ["host", "device", "edited", "compacted", "deeper"])
@pytest.mark.parametrize("scene", ["cube32", "castle"])
def test_every_way_a_tree_gets_into_device_memory(O, H, scenes, scene, state):
    """(b) The answers depend on the voxel set and the depth only — not on who built the records or where they lie."""
    ref = scene_reference(O, scenes, scene)
    pos, mrgb, depth = ref["pos"], ref["mrgb"], ref["depth"]
    rng = np.random.default_rng(5)
    with H.Context(32, 32) as ctx:
        if state == "host":
            ctx.recreate_octree(pos, mrgb)
        elif state == "device":
            ctx.set_voxels_device(pos, mrgb)
        else:
            # half the voxels built (with the ones that fix the depth), the rest added; then a tenth cleared and re-added: holes
            first = rng.random(len(pos)) < 0.5
            first |= (pos.min(1) == pos.min()) | (pos.max(1) == pos.max())
            ctx.recreate_octree(pos[first], mrgb[first])
            assert ctx.scene_depth == depth
            ctx.edit_voxels(pos[~first], mrgb[~first])
            tenth = rng.random(len(pos)) < 0.1
            ctx.clear_voxels(pos[tenth])
            assert ctx.count_voxels() == len(pos) - int(tenth.sum())
            ctx.edit_voxels(pos[tenth], mrgb[tenth])
            storage = ctx.scene_storage()
            assert storage["records_used"] > storage["records_live"]
            if state in ("compacted", "deeper"):
                ctx.compact_scene()
                storage = ctx.scene_storage()
                assert storage["records_used"] == storage["records_live"]
            if state == "deeper":
                # the oracle's tree gets the same depth from an anchor voxel at -(1 << depth); the device gets it by an edit
                ctx.set_scene_depth(depth + 2)
                anchor = np.array([[-(1 << (depth + 2))] * 3], np.int16)
                anchor_mrgb = np.array([[3, 40, 50, 60]], np.uint8)
                ctx.edit_voxels(anchor, anchor_mrgb)
                ref = reference(O, f"{scene}+anchor", np.concatenate([pos, anchor]), np.concatenate([mrgb, anchor_mrgb]), aim=pos)
                assert ref["depth"] == depth + 2
        assert ctx.scene_depth == ref["depth"] and ctx.count_voxels() == len(ref["pos"])
        check_walks(ctx, ref, f"{scene} {state}", only=STATE_FAMILIES)


f32 = np.float32
CAMERAS = {
    "nan_x": (np.array([np.nan, 1, -9], f32), np.array([0.1, -0.05, 1], f32), 1.0),
    "nan_y": (np.array([1, np.nan, -9], f32), np.array([0.1, -0.05, 1], f32), 1.0),
    "on_a_root_face": (np.array([-4, 0.25, 0.25], f32), np.array([1, 0, 0], f32), 1.0),          # cube16's root cube is [-4, 4)^3
    "on_the_centre_planes": (np.array([0, 0, -9], f32), np.array([0, 0, 1], f32), 1.0),
}
FRAME_W, FRAME_H, FRAME_BOUNCES = 32, 24, 3


def oracle_frames(O, scenes, noise, camera, frames):
    key = ("frames", camera)
    if key not in _REF:
        _REF[key] = {}
    ref = scene_reference(O, scenes, "cube16")
    cam = CAMERAS[camera]
    u = O.Uniforms.default()
    u.set_camera(cam[0], O.camera_axis_scaled(cam[0], cam[1], cam[2], FRAME_W, FRAME_H))
    for f in frames:
        if f not in _REF[key]:
            u.frame_number = f
            _REF[key][f] = O.trace(ref["octree"], noise, u, FRAME_W, FRAME_H, FRAME_BOUNCES, crop=(0, 0, FRAME_W, FRAME_H))
    return _REF[key]


TRACERS = [("1", {}), ("4", {}), ("2", {}), ("3", {}), ("5", {}), ("1", {"wide": True}), ("4", {"wide": True}),
           ("1", {"batch": 8}), ("4", {"batch": 8})]


@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("tracer,how", TRACERS, ids=[t + "".join(f"-{k}" for k in how) for t, how in TRACERS])
def test_frames_from_a_camera_the_walk_dislikes(O, H, scenes, noise, monkeypatch, tracer, how, camera):
    """(c) cube16 at 32 x 24, 3 bounces, frames 1 and 2: colour, normal / depth, albedo / leaf word and the ray count against the oracle
    — this reaches the tracers' own calls of the root test (trace_pool.hip, trace_paths.hip, trace_wavefront.hip), which the probes
    do not.  frames_per_launch 8: frames 1 .. 8 in one launch with eight frames of a pixel row per wave, the last one compared."""
    from gpu_voxel_raytracer_amd import TRACE, Camera, Context
    require_variants(H, tracer=tracer, wide="1" if how.get("wide") else None)
    if how.get("wide"):
        monkeypatch.setenv("VXRT_WIDE", "1")
    batch = how.get("batch", 1)
    ref = scene_reference(O, scenes, "cube16")
    want = oracle_frames(O, scenes, noise, camera, range(1, 9) if batch > 1 else (1, 2))

    def compare(ctx, frame, rays):
        for got, exp, label in zip((ctx.read(i) for i in range(3)), want[frame][:3], ("colour", "normal / depth", "albedo / leaf word")):
            assert_bits_equal(got, exp, f"{label}, frame {frame}, tracer {tracer} {how}, camera {camera}")
        assert np.array_equal(ctx.read(2)[..., 3].view(np.uint32), want[frame][2][..., 3].view(np.uint32)), "leaf words"
        assert ctx.stats().rays == rays, "ray count"

    with Context(FRAME_W, FRAME_H, max_bounces=FRAME_BOUNCES, noise=noise, tracer=int(tracer), frames_per_launch=batch) as ctx:
        ctx.recreate_octree(ref["pos"], ref["mrgb"])
        ctx.camera = Camera(*CAMERAS[camera])
        for f in (1, 2):
            ctx.set_frame_number(f - 1)
            ctx.reset_stats()
            ctx.render(TRACE)
            compare(ctx, f, want[f][3])
        if batch > 1:
            ctx.set_frame_number(0)
            ctx.reset_stats()
            ctx.render_frames(TRACE, batch)
            assert ctx.stats().frame_lane_launches >= 1
            compare(ctx, batch, sum(want[f][3] for f in range(1, batch + 1)))
    if camera == "nan_x":        # the shader's root test fails for every primary ray: all sky
        assert (want[1][1][..., 3] == -1).all() and want[1][3] == FRAME_W * FRAME_H
    else:
        assert (want[1][1][..., 3] >= 0).any()
