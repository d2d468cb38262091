"""GPU: every call that changes a loaded scene in place, in one random sequence per start scene (tests/mutator_sequences.py), against
the edit model's dict, the structural checker of the raw records (tests/scene_invariants.py) and a twin context that is given every
step through edit_voxels / clear_voxels / set_scene_depth / fit_scene_depth / compact_scene alone.  A sequence follows an Eulerian
circuit over the fourteen kinds of call (drop_detached and drop_detached_pieces among them), so every kind is directly followed by
every kind (itself included) once, and holds the four batches that end edit_kernel's 1024-segment chunks one short of, at, one past a
full chunk and at two chunks and one.

After every step: get_voxels() equals the model in path order, the decoded records equal the model, the invariants hold with the
build counts the test tracks (taken at the load and after each compaction: nothing changes the counts between a load or a
compaction and the first edit or depth change that takes them), the depth is the model's, and the twin holds the same bytes, stats,
cull box and storage counters.  A compact step equals compact_model on the read-back from before it and leaves tight storage; a
depth or fit step equals scene_depth_model record for record (Tracked.call, which also fails on a shrink the model refuses).  A drop
step's returned tensors are read back and equal what components_model / pieces_model give for its arguments, bit for bit:
positions, bytes and their order, for the pieces also the piece numbers and every field of the table; then the step is checked as
any other (the scene-wide labelling ran on whatever layout the steps before it left, and the steps after it run on what it leaves).
Every fit, and the end of the sequence after a clear of the far voxels, a fit and a compaction, is checked against a fresh context of
the model's list: decoded list, read-back, node count, frames; at the end also records, storage and picks.  On the sponge the first
far_set of each case that has to grow is first made without grow: E_SCENE, and nothing changes; the case asserts that it made the
refusal where its steps hold such a far_set, and the CPU test that the sponge's first case holds one.

The readers.  After those assertions the layout the step left is read through every device reader, with arguments drawn from an rng
of (seed, step index), against the models of the dict and never against the twin, which holds the same bytes (check_readers):
lookup_voxels and count_present of every model voxel (4096 of more), the face neighbours of 256 of them, 256 uniform positions and
64 positions one cell outside each side of the cube, without and with an offset of [-3, 3]^3, against query_model.lookup;
get_voxels_device whole and by a box around a present voxel, and count_voxels of that box, against extract_model's ordered list;
get_voxel_grid of a box of at most 20^3 cells around a present voxel against grid_model.  The one-voxel scene of depth 0 is read in
the same way with the lists its eight cells allow.  At every fit and at the end, pick_device casts the rays of pixel_grid() with a
max_time per ray on the edited context and on the fresh one: the same kernel over two record layouts, the same 36-byte records.

How the circuit is split.  A sequence is 197 circuit steps and 8 boundary steps.  Generating one is a good part of its cost
(the drops' models are union-finds over the whole scene in Python), so MS.part_of generates a sequence only as far as the case at
hand runs, and each case pays for its own steps.  Whole, generated and run, a sequence takes 11.0 s on the sponge, 7.0 s on castle
and 2.7 s on the one-voxel scene (MI355X), where the menger cases of test_gpu_edit.py::test_edits_equal_a_rebuild took 3.09-3.73 s in
the same run.  So each (scene, seed) is PARTS = 5 consecutive cases over the same generated steps (mutator_sequences.PARTS):
1.97-2.37 s each on the sponge, 1.14-1.71 s on castle, 0.25-0.67 s on the one-voxel scene, every one below a menger case of that
test; four parts would put the sponge's at about 2.8 s and leave no room for a slower run.  Scene i's case k takes configuration
(i + k) mod 4, so every scene meets all four.  Case k covers steps [N k / PARTS, N (k + 1) / PARTS) of N = MS.STEPS = 205, the
last case to the sequence's end.  Every case but the first replays the model (not the GPU) and loads that list with
recreate_octree, at the depth the sequence has there (set_scene_depth where that is not the list's own); it starts one step
before its range, so that the ordered pair that straddles two cases is also made on the device directly, not across a rebuild.
The first case loads the scene itself (set_menger for the sponge).

Every assertion message carries the scene, the seed, the step's index, its kind and the kind before it: the steps up to that index
are the reproducible prefix (MS.steps_of(name, seed, index + 1))."""
import contextlib

import numpy as np
import pytest
import torch   # noqa: F401  before the first context: one HIP runtime in the process (host.py: set_voxels_device)

import compact_model as CM
import edit_model as M
import extract_model as X
import grid_model as G
import mutator_sequences as MS
import pieces_model as P
import query_model as Q
import scene_invariants as SI
from test_gpu_compact import assert_tight, pixel_grid, same_arrays
from test_gpu_device_build import STATS, assert_same_scene
from test_gpu_edit import CONFIGS, H_, W, assert_same_frames, fresh, make_ctx   # noqa: F401  (W, H_: the frame the contexts render)
from test_gpu_query import on_device, records
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
    elif a["call"] == "drop_detached":
        got = ctx.drop_detached(a["anchor_min"], a["anchor_max"], connectivity=a["connectivity"])
        assert_returned(got, ("pos", "mrgb"), a)
    elif a["call"] == "drop_detached_pieces":
        got = ctx.drop_detached_pieces(a["anchor_min"], a["anchor_max"], connectivity=a["connectivity"], min_voxels=a["min_voxels"],
                                       max_voxels=a["max_voxels"], cap=a["cap"])
        assert_returned(got[:3], ("pos", "mrgb", "piece"), a)
        assert sorted(got[3]) == sorted(P.FIELDS)
        assert_returned([got[3][f] for f in P.FIELDS], P.FIELDS, a["table"])
    else:
        raise ValueError(a["call"])


def assert_returned(got, names, want):
    """the device tensors a drop returns, read back: the bytes the models give, entry for entry and in their order"""
    for g, name in zip(got, names):
        g, w = g.cpu().numpy(), np.ascontiguousarray(want[name])
        assert g.dtype == w.dtype and g.shape == w.shape, f"the drop's {name}: {g.dtype} {g.shape}, the model has {w.dtype} {w.shape}"
        assert g.tobytes() == w.tobytes(), f"the drop's {name} differs from the model's in {int((g != w).sum())} of {g.size} values"


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


FACES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.int64)


def lookup_positions(keys, depth, rng):
    """int16 [n, 3]: every model voxel (a sample of 4096 of more), the six face neighbours of 256 of those, 256 uniform positions of
    the root cube and 64 one cell outside it on each of its six sides; fewer where the cube has fewer cells (depth 0 has 8)"""
    lim = 1 << depth
    own = keys if len(keys) <= 4096 else keys[rng.choice(len(keys), 4096, replace=False)]
    some = own[rng.choice(len(own), min(256, len(own)), replace=False)]
    parts = [own, (some[:, None, :] + FACES[None, :, :]).reshape(-1, 3), rng.integers(-lim, lim, (min(256, (2 * lim) ** 3), 3))]
    for axis in range(3):
        for at in (-lim - 1, lim):
            p = rng.integers(-lim - 1, lim + 1, (min(64, (2 * lim + 2) ** 2), 3))
            p[:, axis] = at
            parts.append(p)
    return np.clip(np.concatenate(parts), -32768, 32767).astype(np.int16)


def check_readers(ctx, model, depth, ordered, rng):
    """the device readers on the layout the step left, against the models of the dict (never the twin: it holds the same bytes);
    ordered: extract_model.ordered_list(model, depth)"""
    want_pos, want_mrgb = ordered
    keys = want_pos.astype(np.int64)
    # lookup_voxels / count_present
    pos = lookup_positions(keys, depth, rng)
    d_pos = on_device(pos)
    for offset in (None, tuple(int(v) for v in rng.integers(-3, 4, 3))):
        want, present = Q.lookup(model, depth, pos, offset)
        leaf, n = ctx.lookup_voxels(d_pos, offset)
        leaf = leaf.cpu().numpy()
        assert np.array_equal(leaf, want), f"lookup_voxels, offset {offset}: {int((leaf != want).sum())} of {len(pos)} words differ from the model's"
        assert n == present, f"lookup_voxels, offset {offset}: n_present {n}, the model has {present}"
        assert ctx.count_present(d_pos, offset) == present, f"count_present, offset {offset}"
        assert offset is not None or present >= min(len(keys), 4096)
    # get_voxels_device, whole and by a box around a present voxel; count_voxels of that box
    got = [t.cpu().numpy() for t in ctx.get_voxels_device()]
    assert np.array_equal(got[0], want_pos) and np.array_equal(got[1], want_mrgb), "get_voxels_device differs from the model in path order"
    centre = keys[int(rng.integers(len(keys)))]
    lo, hi = centre - rng.integers(0, 12, 3), centre + rng.integers(1, 12, 3)
    inside = X.in_box(want_pos, (lo, hi))
    got = [t.cpu().numpy() for t in ctx.get_voxels_device(lo, hi)]
    assert np.array_equal(got[0], want_pos[inside]) and np.array_equal(got[1], want_mrgb[inside]), f"get_voxels_device of the box {lo} .. {hi}"
    assert ctx.count_voxels(lo, hi) == int(inside.sum()) >= 1, f"count_voxels of the box {lo} .. {hi}"
    # get_voxel_grid of a box of at most 20^3 cells around a present voxel
    dims = rng.integers(1, 21, 3)
    origin = keys[int(rng.integers(len(keys)))] - rng.integers(0, dims)
    inside = X.in_box(want_pos, (origin, origin + dims))
    grid = ctx.get_voxel_grid(tuple(origin.tolist()), tuple(dims.tolist())).cpu().numpy()
    assert np.array_equal(grid, G.list_to_grid(want_pos[inside], want_mrgb[inside], origin, dims)), f"get_voxel_grid of {origin} + {dims}"
    assert np.count_nonzero(grid) == int(inside.sum()) >= 1


def same_bounded_picks(ctx, ref, depth, rng, what):
    """pick_device of the pixel grid's rays with a max_time per ray, on the edited scene and on a fresh build of its voxels: the same
    kernel over two record layouts, the same 36-byte records.  A quarter of the rays are unbounded (2^30, as test_gpu_query.py
    passes it); the others end uniformly within twice the root cube's edge (2^depth world units: a voxel's edge is 0.5), which is
    past its diagonal, so that some end before the cube, some inside it and some beyond."""
    o, d = ctx.pixel_rays(*pixel_grid())
    bound = rng.uniform(0.0, 2.0 * (1 << depth), len(o)).astype(np.float32)
    bound[rng.random(len(o)) < 0.25] = np.float32(Q.UNBOUNDED)
    d_o, d_d, d_t = on_device(o), on_device(d), on_device(bound)
    got, want = records(ctx.pick_device(d_o, d_d, d_t)), records(ref.pick_device(d_o, d_d, d_t))
    differ = np.flatnonzero(got.view(np.uint8).reshape(len(o), -1) != want.view(np.uint8).reshape(len(o), -1))
    assert got.tobytes() == want.tobytes(), f"{what}: bounded pick_device differs from a fresh build's, first at byte {differ[:1]} of {got.itemsize * len(o)}"


def check_step(ctx, twin, model, depth, built, rng):
    svo, leaves = ctx.read_scene()
    assert ctx.scene_depth == depth, f"scene_depth {ctx.scene_depth}, the model expects {depth}"
    SI.check(svo, leaves, depth, ctx.scene_storage(), ctx.stats().octree_nodes, built=built)
    assert M.decode_records(svo, leaves, depth) == model, "the decoded records differ from the model"
    pos, mrgb = ctx.get_voxels()
    want_pos, want_mrgb = X.ordered_list(model, depth)
    assert np.array_equal(pos, want_pos) and np.array_equal(mrgb, want_mrgb), "get_voxels differs from the model in path order"
    assert_same_scene(ctx, twin, "the host twin")
    assert ctx.scene_storage() == twin.scene_storage(), ("the host twin's storage", ctx.scene_storage(), twin.scene_storage())
    check_readers(ctx, model, depth, (want_pos, want_mrgb), rng)


@pytest.mark.parametrize("name, seed, part, cfg", CASES, ids=["%s-seed%d-part%d-tracer%d-cull%d-fif%d-fpl%d" % ((n, s, p) + c) for n, s, p, c in CASES])
def test_every_mutator_after_every_other(H, scenes, name, seed, part, cfg):
    start, depth, steps, first, last = MS.part_of(name, seed, part)      # one step of overlap: see above
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
            check_step(ctx, twin, model, depth, built, np.random.default_rng((seed, first, 1)))
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
                rng = np.random.default_rng((seed, i))
                check_step(ctx, twin, model, depth, built, rng)
                if s.kind == "fit":
                    check_rebuild(H, ctx, model, cam, cfg, 3 + 2 * (i % 7), where,
                                  also=lambda ref: same_bounded_picks(ctx, ref, depth, rng, "after the fit"))
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
            rng = np.random.default_rng((seed, len(steps), 2))
            check_step(ctx, twin, model, depth, built, rng)
            assert_tight(ctx, "the end")
            check_rebuild(H, ctx, model, cam, cfg, 5, "the end")
            with fresh(H, cfg, model, cam) as ref:
                assert_same_scene(ctx, ref, "against a fresh build")
                assert ctx.scene_storage() == ref.scene_storage()
                got, want = ctx.pick_pixels(*pixel_grid()), ref.pick_pixels(*pixel_grid())
                for key in want:
                    assert np.array_equal(got[key].view(np.uint8), want[key].view(np.uint8)), f"pick_pixels: {key}"
                same_bounded_picks(ctx, ref, depth, rng, "the end")
