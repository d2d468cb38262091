"""CPU: the generator of the mutator sequences (tests/mutator_sequences.py), for every start scene and seed the GPU test uses: the pair
coverage, the legality of every step against the model alone, the chunk-boundary batches, the two drops against components_model and
pieces_model, and that no step passes for coverage while doing nothing."""
import numpy as np
import pytest

import components_model as K
import edit_model as M
import mutator_sequences as MS
import pieces_model as P
import solid_model as S
import voxelize_model as V


@pytest.fixture(scope="module", params=MS.CASES, ids=lambda c: f"{c[0]}-seed{c[1]}")
def replay(request):
    """-> (name, start model, [(step, model before it, depth before it)], final model, (name, seed))"""
    name, seed = request.param
    model, depth, steps = MS.steps_of(name, seed)
    m, rows = dict(model), []
    for s in steps:
        rows.append((s, dict(m), depth))
        s.apply_to_model(m)
        depth = s.args["depth"]
    return name, model, rows, m, (name, seed)


def test_every_ordered_pair_occurs(replay):
    _, _, rows, _, _ = replay
    kinds = [s.kind for s, _, _ in rows]
    assert set(kinds) == set(MS.KINDS)
    pairs = set(zip(kinds, kinds[1:]))
    assert pairs == {(a, b) for a in MS.KINDS for b in MS.KINDS}
    # the circuit itself, without the inserted boundary batches: 197 steps, every pair exactly once
    assert len(MS.KINDS) == 14
    own = [s.kind for s, _, _ in rows if "boundary" not in s.args][:197]
    assert len(own) == 197 and len(set(zip(own, own[1:]))) == 196


def test_the_parts_cover_the_sequence(replay):
    """the GPU test's cases: consecutive ranges with one step of overlap, the last to the sequence's end, each generated only as far
    as its own last step"""
    _, _, rows, _, (name, seed) = replay
    assert len(rows) in (MS.STEPS, MS.STEPS + 1) and MS.STEPS == 205
    ends = 0
    for part in range(MS.PARTS):
        _, _, steps, first, last = MS.part_of(name, seed, part)
        assert first == max(ends - 1, 0) and first < last <= len(steps)
        assert [s.kind for s in steps[:last]] == [s.kind for s, _, _ in rows[:last]]
        ends = last
    assert ends == len(rows)
    fresh = MS.sequence(seed, rows[0][1], rows[0][2])               # generated step by step: the same steps as generated whole
    for (s, _, _), again in zip(rows[:12], fresh):
        assert s.kind == again.kind and s.args["depth"] == again.args["depth"] and len(s.args["twin"]) == len(again.args["twin"])


def test_the_circuit_is_eulerian_for_any_seed():
    for seed in range(20):
        order = MS.circuit(np.random.default_rng(seed))
        assert len(order) == 197 and sorted(zip(order, order[1:])) == sorted((a, b) for a in MS.KINDS for b in MS.KINDS)


def positions_of(step):
    return [(t[0], np.asarray(t[1], np.int64).reshape(-1, 3)) for t in step.args["twin"] if t[0] in ("set", "clear")]


def test_every_step_is_legal_against_the_model(replay):
    _, _, rows, _, _ = replay
    shrinks = grows = 0
    for i, (s, before, depth) in enumerate(rows):
        what = (i, s.kind)
        after_depth = s.args["depth"]
        assert 0 <= depth <= 15 and 0 <= after_depth <= 15, what
        # positions: inside the cube the step starts in, unless it grows; what it sets inside the cube it ends in
        for op, p in positions_of(s):
            for d in ([] if s.args["grows"] else [depth]) + ([after_depth] if op == "set" else []):
                assert np.all((p >= -(1 << d)) & (p < (1 << d))), what
        after = s.apply_to_model(dict(before))
        if after and s.kind not in ("fit",):
            assert MS.holding_depth(after) <= after_depth, what           # a depth step that shrinks is a legal shrink
        if s.kind == "fit":
            assert after_depth == MS.natural_depth(after), what
        elif s.kind == "depth":
            assert after_depth == s.args["to"], what
            shrinks += after_depth < depth
        elif not s.args["grows"]:
            assert after_depth == depth, what
        else:
            assert after_depth >= depth, what
            grows += after_depth > depth
        if s.kind in ("compact", "depth"):
            assert after == before, what
    assert shrinks >= 1 and grows >= 3                                    # set_scene_depth shrinks, and the grow=True forms grow
    depths = [depth for _, _, depth in rows] + [rows[-1][0].args["depth"]]
    assert any(s.kind == "far_set" and after > before for (s, _, before), after in zip(rows, depths[1:]))   # the refusal's step
    if replay[0] == "menger_device":          # the GPU test makes the refusal in every case whose steps hold one: the first does
        steps = [s for s, _, _ in rows]
        assert MS.part_of(*replay[4], 0)[3:] == MS.part_range(MS.STEPS, 0)
        at = MS.refusal_step(steps, rows[0][2], *MS.part_range(MS.STEPS, 0))
        assert at is not None and steps[at].kind == "far_set" and steps[at].args["depth"] > rows[at][2]


def test_the_boundary_batches(replay):
    _, _, rows, _, _ = replay
    kinds = [s.kind for s, _, _ in rows]
    first_compact = kinds.index("compact")
    counts = []
    for i, (s, before, depth) in enumerate(rows):
        if "boundary" not in s.args or not s.kind.startswith("set"):
            continue
        assert i > first_compact
        pos = s.args["pos"].astype(np.int64)
        n = s.args["boundary"]
        counts.append(n)
        assert np.all(pos % 2 == 0)
        parents = {tuple(p) for p in (pos >> 1).tolist()}
        assert len(pos) == len(parents) == n
        assert not parents & {(x >> 1, y >> 1, z >> 1) for x, y, z in before}
        nxt = rows[i + 1][0]
        assert nxt.kind == s.kind.replace("set", "clear") and nxt.args["boundary"] == n and np.array_equal(nxt.args["pos"], s.args["pos"])
        assert rows[i + 2][1] == before                                   # set and cleared again: the model as before
    assert sorted(counts) == sorted(MS.BOUNDARY_COUNTS)


def voxel_bytes(model):
    """the edit model's dict as the components and pieces models take it: {pos: (m, r, g, b)}"""
    pos, mrgb = M.to_list(model)
    return {tuple(p): tuple(c) for p, c in zip(pos.tolist(), mrgb.tolist())}


def test_the_drops_equal_the_models(replay):
    """every drop step: its arguments are legal, what it says the call returns is the model's list for those arguments, and its
    effect is the clear of that list; per sequence the drops do remove something, by both calls, and leave KEEP voxels"""
    _, _, rows, _, _ = replay
    removed = {"drop_detached": 0, "drop_detached_pieces": 0}
    some_left_behind = 0
    for i, (s, before, depth) in enumerate(rows):
        if s.kind not in removed:
            continue
        what, a = (i, s.kind), s.args
        assert a["call"] == s.kind and a["connectivity"] in (6, 18, 26) and a["depth"] == depth and not a["grows"], what
        lo, hi = a["anchor_min"], a["anchor_max"]
        assert all(-32768 <= l <= h <= 32768 for l, h in zip(lo, hi)), what
        assert sum((l, h) != (-32768, 32768) for l, h in zip(lo, hi)) <= 1, what                    # a half-space
        voxels = voxel_bytes(before)
        if s.kind == "drop_detached":
            want = K.detached(voxels, lo, hi, a["connectivity"])
        else:
            most = P.EVERY if a["max_voxels"] is None else a["max_voxels"]
            want = P.detached_pieces(voxels, lo, hi, a["connectivity"], a["min_voxels"], most)
            assert np.array_equal(a["piece"], want[2]) and a["piece"].dtype == np.uint32, what
            assert a["table"].dtype == P.PIECE and a["table"].tobytes() == want[3].tobytes(), what
            assert a["cap"] is None or len(want[0]) <= a["cap"] <= len(want[0]) + 5, what             # never below the count
            every = P.detached_pieces(voxels, lo, hi, a["connectivity"])[3]["voxels"].tolist()
            if len(set(every)) >= 2:
                assert 0 < len(want[3]) < len(every), what
            some_left_behind += 0 < len(want[3]) < len(every)
        assert np.array_equal(a["pos"], want[0]) and a["pos"].dtype == np.int16, what
        assert np.array_equal(a["mrgb"], want[1]) and a["mrgb"].dtype == np.uint8, what
        gone = set(map(tuple, a["pos"].tolist()))
        assert len(gone) == len(a["pos"]) and gone <= set(before), what
        after = s.apply_to_model(dict(before))
        assert after == {p: w for p, w in before.items() if p not in gone}, what
        assert a["twin"] == ([("clear", a["pos"])] if len(gone) else []), what
        assert len(after) >= MS.KEEP, what
        removed[s.kind] += len(gone) > 0
    assert removed["drop_detached"] >= 1 and removed["drop_detached_pieces"] >= 1 and some_left_behind >= 1, (removed, some_left_behind)


def test_no_step_counts_without_doing_something(replay):
    _, _, rows, final, _ = replay
    for i, (s, before, depth) in enumerate(rows):
        after = s.apply_to_model(dict(before))
        if s.kind in ("mesh", "carve", "set_host", "set_device", "far_set"):
            assert after != before, (i, s.kind)
        if s.kind == "carve":
            assert len(after) < len(before)
        assert after, (i, s.kind)
    assert final
    name, model = replay[0], replay[1]
    assert len(final) - len(MS.far_voxels(final, MS.core_depth(model))) >= 1


def test_moved_shapes_equal_the_models_of_the_moved_meshes():
    """the generator voxelises each shape once and moves the lists by whole voxels: the rules commute with that"""
    as_set = lambda p: set(map(tuple, np.asarray(p, np.int64).tolist()))   # noqa: E731
    for (name, radius), shift in ((("icosphere1", 3), (5, -7, 100)), (("icosphere2", 2), (-33, 0, 1)), (("cube", 3), (-4, 9, 2))):
        v, t, surface, inner = MS.shape(name, radius)
        moved = (v.astype(np.float64) + np.array(shift)).astype(np.float32)
        assert as_set(V.voxelize(moved, t, (1, 2, 3, 4))[0]) == as_set(surface + np.array(shift))
        assert as_set(S.solid(moved, t, None, (0, 0, 0, 0), interior_only=True)[0]) == as_set(inner + np.array(shift))
        pos, mrgb = S.solid(moved, t, np.array([1, 2, 3, 4], np.uint8), (5, 6, 7, 8))
        upos, umrgb = MS.union_list(surface + np.array(shift), inner + np.array(shift), (1, 2, 3, 4), (5, 6, 7, 8))
        assert M.from_list(pos, mrgb) == M.from_list(upos, umrgb)
