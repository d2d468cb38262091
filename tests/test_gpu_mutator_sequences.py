"""GPU: every call that changes a loaded scene in place, in one random sequence per start scene (tests/mutator_sequences.py), against
the edit model's dict, the structural checker of the raw records (tests/scene_invariants.py) and a twin context that is given every
step through edit_voxels / clear_voxels / set_scene_depth / fit_scene_depth / compact_scene alone.  A sequence follows an Eulerian
circuit over the twelve kinds of call, so every kind is directly followed by every kind (itself included) once, and holds the four
batches that end edit_kernel's 1024-segment chunks one short of, at, one past a full chunk and at two chunks and one.

After every step: get_voxels() equals the model in path order, the decoded records equal the model, the invariants hold with the
build counts the test tracks (taken at the load and after each compaction: nothing changes the counts between a load or a
compaction and the first edit or depth change that takes them), the depth is the model's, and the twin holds the same bytes, stats,
cull box and storage counters.  A compact step equals compact_model on the read-back from before it and leaves tight storage; a
depth or fit step equals scene_depth_model record for record (Tracked.call, which also fails on a shrink the model refuses).  Every
fit, and the end of the sequence after a clear of the far voxels, a fit and a compaction, is checked against a fresh context of the
model's list: decoded list, read-back, node count, frames; at the end also records, storage and picks.  On the sponge the first
far_set of each case that has to grow is first made without grow: E_SCENE, and nothing changes; the case asserts that it made the
refusal where its steps hold such a far_set, and the CPU test that the sponge's first case holds one.

How the circuit is split.  A sequence is 145 circuit steps and 8 boundary steps.  Whole, it takes 5.7 s on the sponge, 5.0 s on castle
and 2.2 s on the one-voxel scene (MI355X), where the cases of test_gpu_edit.py::test_edits_equal_a_rebuild take 3.3-3.6 s on menger
(and 14.5-20.4 s on the start-up scene, under 1.9 s on castle and the sponge).  So each (scene, seed) is PARTS = 2 consecutive cases
over the same generated steps (mutator_sequences.PARTS), 0.65-2.98 s each, every one below a menger case of that test; four parts
would cost two more rebuilds per scene and buy nothing.  Two cases per scene also let the three scenes use all four configurations
between them: (scene index + part) mod 4, so 0 and 1, 1 and 2, 2 and 3.  Case k
covers steps [N k / PARTS, N (k + 1) / PARTS).  The second case replays the model (not the GPU) and loads that list with
recreate_octree, at the depth the sequence has there (set_scene_depth where that is not the list's own); it starts one step
before its range, so that the ordered pair that straddles the two cases is also made on the device directly, not across a rebuild.
The first case loads the scene itself (set_menger for the sponge).

Every assertion message carries the scene, the seed, the step's index, its kind and the kind before it: the steps up to that index
are the reproducible prefix (MS.steps_of(name, seed))."""
import contextlib

import numpy as np
import pytest
import torch   # noqa: F401  before the first context: one HIP runtime in the process (host.py: set_voxels_device)

import compact_model as CM
import edit_model as M
import extract_model as X
import mutator_sequences as MS
import scene_invariants as SI
from test_gpu_compact import assert_tight, pixel_grid, same_arrays
from test_gpu_device_build import STATS, assert_same_scene
from test_gpu_edit import CONFIGS, H_, W, assert_same_frames, fresh, make_ctx   # noqa: F401  (W, H_: the frame the contexts render)
from test_gpu_scene_depth import Tracked, check_rebuild

pytestmark = pytest.mark.gpu

PARTS = MS.PARTS
CASES = [(name, seed, part, CONFIGS[(i + part) % len(CONFIGS)]) for i, (name, seed) in enumerate(MS.CASES) for part in range(PARTS)]


@contextlib.contextmanager
def at(where):
    """an assertion that fails inside names the step"""
    try:
        yield
    except Exception as e:      # a failed check, a shrink the model refuses, a call the library refuses
        raise AssertionError(f"{where}: {type(e).__name__}: {e}") from e


def camera_of(scenes, name):
    if name == "menger_device":
        return scenes.close_camera((27, 27, 27))
    if name == "one_voxel":
        return (0.3, 0.4, -3.0), (0.0, 0.0, 1.0), 1.0
    return scenes.close_camera(scenes.load_scene(name)[2])


def load(H, scenes, ctx, name, part, model, depth):
    """the start scene itself for the first part, the replayed model's list at the sequence's depth for the others -> build counts"""
    if part == 0 and name == "menger_device":
        ctx.set_menger(3, 0, MS.MENGER_MRGB)
    elif part == 0:
        ctx.recreate_octree(*MS.start_model(H, scenes, name)[:2])
    else:
        ctx.recreate_octree(*M.to_list(model))
    svo, leaves = ctx.read_scene()
    if ctx.scene_depth != depth:
        ctx.set_scene_depth(depth)
    return len(svo), len(leaves)


def snapshot(ctx):
    st = ctx.stats()
    return (ctx.read_scene(), ctx.scene_storage(), [getattr(st, f) for f in STATS], list(st.cull_box_min), list(st.cull_box_max))


def same_snapshot(a, b):
    return same_arrays(a[0], b[0]) and a[1:] == b[1:]


def call(ctx, step, grow=None):
    """the step's own call on the context (depth, fit and compact steps are made by the test itself)"""
    a = step.args
    grow = a.get("grow", False) if grow is None else grow
    if a["call"] == "host":
        ctx.edit_voxels(a["pos"], a["mrgb"], grow=grow) if "mrgb" in a else ctx.clear_voxels(a["pos"])
    elif a["call"] == "device":
        ctx.edit_voxels_device(a["pos"], a["mrgb"], grow=grow) if "mrgb" in a else ctx.clear_voxels_device(a["pos"])
    elif a["call"] == "grid":
        ctx.edit_voxel_grid(a["cells"], a["origin"], mode=a["mode"], grow=grow)
    elif a["call"] == "mesh":
        ctx.edit_mesh(a["verts"], a["tris"], a["mrgb"], grow=grow)
    elif a["call"] == "solid":
        ctx.edit_solid(a["verts"], a["tris"], a["mrgb"], a["fill"], grow=grow)
    elif a["call"] == "carve":
        ctx.carve_solid(a["verts"], a["tris"])
    else:
        raise ValueError(a["call"])


def call_twin(twin, step):
    for t in step.args["twin"]:
        if t[0] == "set":
            twin.edit_voxels(t[1], t[2])
        elif t[0] == "clear":
            twin.clear_voxels(t[1])
        elif t[0] == "depth":
            twin.set_scene_depth(t[1])
        elif t[0] == "fit":
            twin.fit_scene_depth()
        else:
            twin.compact_scene()


def check_step(ctx, twin, model, depth, built):
    svo, leaves = ctx.read_scene()
    assert ctx.scene_depth == depth, f"scene_depth {ctx.scene_depth}, the model expects {depth}"
    SI.check(svo, leaves, depth, ctx.scene_storage(), ctx.stats().octree_nodes, built=built)
    assert M.decode_records(svo, leaves, depth) == model, "the decoded records differ from the model"
    pos, mrgb = ctx.get_voxels()
    want_pos, want_mrgb = X.ordered_list(model, depth)
    assert np.array_equal(pos, want_pos) and np.array_equal(mrgb, want_mrgb), "get_voxels differs from the model in path order"
    assert_same_scene(ctx, twin, "the host twin")
    assert ctx.scene_storage() == twin.scene_storage(), ("the host twin's storage", ctx.scene_storage(), twin.scene_storage())


@pytest.mark.parametrize("name, seed, part, cfg", CASES, ids=["%s-seed%d-part%d-tracer%d-cull%d-fif%d-fpl%d" % ((n, s, p) + c) for n, s, p, c in CASES])
def test_every_mutator_after_every_other(H, scenes, name, seed, part, cfg):
    start, depth, steps = MS.steps_of(name, seed)
    first, last = MS.part_range(len(steps), part)      # one step of overlap: see above
    refusal = MS.refusal_step(steps, depth, first, last) if name == "menger_device" else None
    model = dict(start)
    for s in steps[:first]:
        s.apply_to_model(model)
        depth = s.args["depth"]
    cam = camera_of(scenes, name)
    refused = False
    with make_ctx(H, cfg) as ctx, make_ctx(H, cfg) as twin:
        built = load(H, scenes, ctx, name, part, model, depth)
        assert load(H, scenes, twin, name, part, model, depth) == built
        ctx.camera = H.Camera(*cam)
        with at(f"{name} seed {seed}: loaded for step {first}"):
            check_step(ctx, twin, model, depth, built)
        for i in range(first, last):
            s = steps[i]
            where = f"{name} seed {seed} step {i} {s.kind} (after {steps[i - 1].kind if i > first else 'the load'})"
            with at(where):
                if i == refusal:
                    assert s.kind == "far_set" and s.args["depth"] > depth
                    before = snapshot(ctx)
                    with pytest.raises(H.VxrtError) as e:
                        call(ctx, s, grow=False)
                    assert e.value.status == H.E_SCENE
                    assert same_snapshot(snapshot(ctx), before), "the refused call changed the scene"
                    refused = True
                if s.kind == "compact":
                    before = ctx.read_scene()
                    ctx.compact_scene()
                    assert same_arrays(ctx.read_scene(), CM.compact(*before, depth)), "device records differ from compact_model's"
                    assert_tight(ctx, where)
                elif s.kind in ("depth", "fit"):
                    if s.kind == "fit" and len(s.args["clear"]):
                        ctx.clear_voxels(s.args["clear"])
                    t = Tracked(ctx)
                    t.built = built
                    assert t.call(s.args["to"] if s.kind == "depth" else None) == s.args["depth"]
                else:
                    call(ctx, s)
                call_twin(twin, s)
                s.apply_to_model(model)
                depth = s.args["depth"]
                if s.kind == "compact":
                    built = tuple(len(a) for a in ctx.read_scene())
                check_step(ctx, twin, model, depth, built)
                if s.kind == "fit":
                    check_rebuild(H, ctx, model, cam, cfg, 3 + 2 * (i % 7), where)
        assert refused == (refusal is not None), f"{name} seed {seed}: the refusal at step {refusal} was not made"
        if part != PARTS - 1:
            return
        # the end of the sequence: the far voxels cleared, the depth fitted, the storage compacted: a fresh build, byte for byte
        with at(f"{name} seed {seed}: the end, after step {last - 1} {steps[-1].kind}"):
            far = MS.far_voxels(model, MS.core_depth(start))
            for c in (ctx, twin):
                if len(far):
                    c.clear_voxels(far)
                c.fit_scene_depth()
                c.compact_scene()
            M.apply(model, far, None)
            assert model
            depth = H.scene_depth_for(M.to_list(model)[0])
            built = tuple(len(a) for a in ctx.read_scene())
            check_step(ctx, twin, model, depth, built)
            assert_tight(ctx, "the end")
            check_rebuild(H, ctx, model, cam, cfg, 5, "the end")
            with fresh(H, cfg, model, cam) as ref:
                assert_same_scene(ctx, ref, "against a fresh build")
                assert ctx.scene_storage() == ref.scene_storage()
                got, want = ctx.pick_pixels(*pixel_grid()), ref.pick_pixels(*pixel_grid())
                for key in want:
                    assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), f"pick_pixels: {key}"
