"""CPU: the families of tests/list_families.py are what they claim, by the models alone, and every family goes through the three
host-compiled rule programs (test_morph_cpu.DRIVER, test_mesh_cpu.DRIVER, test_setops_cpu.DRIVER: each a program of its own, built
under the undefined-behaviour and address sanitizers) against the models bit for bit.

A claim that is a count or a share is held to list_families.FLOOR; the claims below that are not hold exactly.  What goes through
the rule programs: every case of every family through the morphology's at one connectivity, rotating over those the case is allowed
(list_families.connectivities: 6 alone above 5 000 distinct cells and for the full bars), all four ops; every case through the
mesher's in both modes with bytes (the full bars in RUNS mode, and the first in FACES mode too: a bar's FACES mesh is the same on
every axis and in every colouring but for the axes' order and the bytes); of the full bars the three of one colour, one of period
2 047 and one whose colours differ in bit 7, each through two of the four ops (CPU_MORPH_BARS); every pair through the combiner's,
both ways round, all five ops."""
import numpy as np
import pytest

import list_families as F
import mesh_model as MM
import morph_model as M
import setops_model as S
import test_mesh_cpu
import test_morph_cpu
import test_setops_cpu
from transform_families import path_keys
from transform_model import HI, LO, source_of


def floor(family, claim, value):
    assert value >= F.FLOOR[(family, claim)], (family, claim, value)


def every_pair(cells, offset):
    """-> the distinct cells whose cell at `offset` is listed too"""
    return cells[F.listed_neighbour(cells, offset)]


def step_bits(cells, offset):
    """Per cell and axis the bits the step by `offset` carries (+ 1: the ones at u's low end) or borrows (- 1: the zeros), -1 where
    the axis stands still."""
    u = F.u_of(cells)
    o = np.asarray(offset)
    return np.where(o > 0, F.trailing_ones(u), np.where(o < 0, F.trailing_zeros(u), -1))


# ---- seams ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seam_cells():
    return F.distinct(np.concatenate([c.pos for c in F.seams()]))


def test_seams_step_across_every_carry_and_borrow(seam_cells):
    assert len(F.seam_centres()) == 1 + 15 * 2 * 4 + 100
    for axis in range(3):
        for d, bits in ((1, F.trailing_ones), (-1, F.trailing_zeros)):
            o = [0, 0, 0]
            o[axis] = d
            seen = set(bits(F.u_of(every_pair(seam_cells, o))[:, axis]).tolist())
            assert set(range(16)) <= seen, (axis, d, sorted(set(range(16)) - seen))
    # diagonal steps (rows 6 to 25) that carry k bits on exactly two axes at once, and others on three: the offsets without a - 1,
    # so that every moving axis carries; then the same for borrows, the offsets without a + 1
    for sign, what in ((1, "carry"), (-1, "borrow")):
        two, three = set(), set()
        for o in M.OFFSETS[6:]:
            if -sign in o:
                continue
            got = step_bits(every_pair(seam_cells, o), o)
            for k in range(6, 15):
                n = (got == k).sum(axis=1)
                if (n == 2).any():
                    two.add(k)
                if (n == 3).any():
                    three.add(k)
        assert two == set(range(6, 15)) and three == set(range(6, 15)), (what, sorted(two), sorted(three))
    wide = 0
    for o in M.OFFSETS:
        got = step_bits(every_pair(seam_cells, o), o)
        wide += int(((got >= 6) & (got <= 14)).any(axis=1).sum())
    floor("seams", "listed pairs one step apart whose step carries or borrows 6 to 14 bits", wide)


def test_seams_clusters_and_middle_bits(seam_cells):
    cube = F._block(4) - 2
    listed = set(map(tuple, seam_cells.tolist()))
    share = np.mean([[tuple(v) in listed for v in (cube + np.array(c)).tolist()] for c in F.seam_centres()])
    floor("seams", "occupancy of a cluster's 4^3 cells", float(share))
    middle = (F.u_of(seam_cells) >> 6) & 0x1FF
    floor("seams", "distinct patterns of bits 6 to 14 of u, over the three axes", len(set(middle.reshape(-1).tolist())))
    for case in F.seams():
        assert len(case.pos) > len(F.distinct(case.pos)) and case.name.startswith("seams[") and str(F.SEED) in case.name


# ---- range_faces ---------------------------------------------------------------------------------------------------------------------
def test_range_faces_has_an_outside_neighbour_at_every_row():
    outside_any = 0
    for case in F.range_faces():
        cells = F.distinct(case.pos)
        for r, o in enumerate(M.OFFSETS):
            q = cells + np.array(o)
            outside = ~((q >= LO) & (q <= HI)).all(axis=1)
            opposite = F.listed_neighbour(cells, tuple(-v for v in o))
            assert (outside & opposite).any(), (case.name, r, o)
        q = cells[:, None, :] + np.array(M.OFFSETS)[None, :, :]
        outside_any += int((~((q >= LO) & (q <= HI)).all(axis=2)).any(axis=1).sum())
        listed = set(map(tuple, cells.tolist()))
        patches = len(M.OFFSETS)
        assert len(cells) <= 27 * patches
        floor("range_faces", "occupancy of a patch's 3^3 cells", len(listed) / (27 * patches))
        # a corner coordinate of 65 536 (bit 16 of a corner key's field) and a plane at 65 536 (bit 16 of a face key's w), on each axis
        verts = F.meshed("range_faces", F.range_faces().index(case), MM.RUNS)[0]
        assert verts.max(axis=0).tolist() == [32768.0] * 3 and verts.min(axis=0).tolist() == [-32768.0] * 3
        planes = {(MM.axis_of(d), w) for (d, w, _, _), _ in MM.faces_of(source_of(case.pos, case.mrgb))}
        assert {(a, 32768) for a in range(3)} <= planes
    floor("range_faces", "listed voxels with a neighbour outside the range", outside_any)


# ---- far -----------------------------------------------------------------------------------------------------------------------------
def both_values(keys, bits):
    keys = np.asarray(keys, np.int64)
    return [b for b in range(bits) if not (0 < int(((keys >> b) & 1).sum()) < len(keys))]


def test_far_uses_every_bit_of_the_keys():
    for k, case in enumerate(F.far()):
        cells = F.distinct(case.pos)
        assert len(cells) == F.FAR_SIZES[k] and len(case.pos) <= F.MAX_LIST
        assert both_values(path_keys(cells), 48) == [], case.name
        alone = ~np.any([F.listed_neighbour(cells, o) for o in M.OFFSETS], axis=0)
        floor("far", "share of voxels without a listed neighbour at connectivity 26", float(alone.mean()))
        assert alone.mean() < 1.0
        floor("far", "distinct patterns of bits 6 to 14 of u on one axis", min(len(set(((F.u_of(cells)[:, a] >> 6) & 0x1FF).tolist())) for a in range(3)))
    # the 52 bits of the face keys among the model's faces and the 51 of the corner keys among its corners, but for bit 16 of w and
    # of a corner's field, which only 65 536 sets: test_range_faces_has_an_outside_neighbour_at_every_row
    case = F.far()[1]
    faces = np.array([f for f, _ in MM.faces_of(source_of(case.pos, case.mrgb))], np.int64)
    face_keys = faces[:, 0] << 49 | (faces[:, 1] + 32768) << 32 | (faces[:, 2] + 32768) << 16 | (faces[:, 3] + 32768)
    assert set(both_values(face_keys, 52)) <= {48}, both_values(face_keys, 52)
    corners = F.meshed("far", 1, MM.FACES)[0].astype(np.int64) + 32768
    corner_keys = corners[:, 0] << 34 | corners[:, 1] << 17 | corners[:, 2]
    assert set(both_values(corner_keys, 51)) <= {16, 33, 50}, both_values(corner_keys, 51)


# ---- sizes, vertex_counts -------------------------------------------------------------------------------------------------------------
def test_sizes_have_exactly_the_counts_named():
    counts = F.size_counts()
    assert len(counts) == 44 and {1, 2, 3, 2047, 2048, 2049, 6143, 6144, 6145, 8191, 8192, 8193, 16383, 16384, 16385} <= set(counts)
    assert all({(1 << k) - 1, 1 << k, (1 << k) + 1} <= set(counts) for k in range(1, 15)) and all({2048 * j - 1, 2048 * j, 2048 * j + 1} <= set(counts) for j in range(1, 5))
    again = []
    for m, case in zip(counts, F.sizes()):
        cells = F.distinct(case.pos)
        assert len(cells) == m and len(source_of(case.pos)) == m and m < len(case.pos) <= F.MAX_LIST, case.name
        assert m < 8 or (cells.min() < 0 <= cells.max() and 8 * m <= (2 * max(-cells.min(), cells.max() + 1)) ** 3), case.name      # sparse, across the origin
        again.append((len(case.pos) - m) / len(case.pos))
    floor("sizes", "share of entries that list a position again", float(np.mean(again[10:])))


def test_vertex_counts_have_exactly_the_counts_named():
    targets = list(F.vertex_reachable())
    assert set(F.vertex_targets()) - set(targets) == {7, 9, 17} and sorted(F._pieces()) == [8, 14, 15, 19, 23]
    assert all(F._solve(t) is None for t in F.UNREACHABLE)
    assert len(F.vertex_counts()) == len(targets) == 30
    for k, (target, case) in enumerate(zip(targets, F.vertex_counts())):
        for mode in MM.MODES:                      # at least one case per mode: every case in both, with and without bytes
            for bare in (False, True):
                assert len(F.meshed("vertex_counts", k, mode, bare)[0]) == target, (case.name, MM.NAMES[mode], bare)


# ---- long_runs -----------------------------------------------------------------------------------------------------------------------
def test_long_runs_are_in_order_and_as_long_as_the_header_allows():
    assert [kind for kind, _, _ in F.LONG_KINDS].count("period") == len(F.PERIODS) and {a for kind, a, _ in F.LONG_KINDS if kind == "period"} == {0, 1, 2}
    for (kind, axis, period), case in zip(F.LONG_KINDS, F.long_runs()):
        assert len(case.pos) == F.BAR == len(F.distinct(case.pos)) and case.pos[:, axis].tolist() == list(range(LO, HI + 1))
        words = case.mrgb.astype(np.int64) @ np.array([1 << 24, 1 << 16, 1 << 8, 1])
        if kind == "one colour":
            assert max(MM.quad_areas(case.pos, case.mrgb, MM.RUNS)) == F.BAR and len(set(words.tolist())) == 1
        if kind == "bit 7":
            # the colours differ in bit 7 of the material byte and nowhere else: no run breaks
            assert len(set(words.tolist())) == 2 and len(set((words & 0x7FFFFFFF).tolist())) == 1
            assert len(F.meshed("long_runs", F.LONG_KINDS.index((kind, axis, period)), MM.RUNS)[1]) == 2 * (2 + 2 * F.BAR + 2)


def test_the_bar_piece_changes_colour_and_dilates_twice():
    piece = F.bar_piece()
    k, lo, hi = F.PIECE
    assert F.LONG_KINDS[k] == ("period", 2, 2047) and len(piece.pos) == hi - lo == 2 * F.SPAN + 1 and np.array_equal(piece.pos, F.long_runs()[k].pos[lo:hi])
    changes = int((piece.mrgb[1:] != piece.mrgb[:-1]).any(axis=1).sum())
    assert changes == 3
    once, twice = F.morphed_piece(M.DILATE, 6, 1), F.morphed_piece(M.DILATE, 6, 2)
    assert len(once[0]) == 5 * len(piece.pos) + 2 and len(twice[0]) == 13 * len(piece.pos) + 12 and len(F.morphed_piece(M.MARGIN, 6, 2)[0]) == len(twice[0]) - len(piece.pos)
    assert len({tuple(b) for b in twice[1].tolist()}) == 3


@pytest.mark.parametrize("k", [k for k, (kind, _, _) in enumerate(F.LONG_KINDS) if kind == "period"], ids=lambda k: f"period {F.LONG_KINDS[k][2]}")
def test_a_periods_heads_stand_on_both_sides_of_a_block(k):
    _, axis, period = F.LONG_KINDS[k]
    case = F.long_runs()[k]
    faces = MM.faces_of(source_of(case.pos, case.mrgb))
    d = (axis + 1) % 3
    assert [f[0][0] for f in faces].index(d) == F.run_base(axis) and faces[F.run_base(axis) + F.BAR - 1][0][0] == d
    heads, at = [], 0
    for q in MM.quads_of(faces, MM.RUNS, True):
        heads.append(at)
        at += q[4] - q[3]
    assert at == len(faces)
    # the heads that a change of colour makes: the face before is the same row's cell before
    made = {i for i in heads if i and faces[i - 1][0] == (*faces[i][0][:3], faces[i][0][3] - 1)}
    assert any(i % F.SPAN == F.SPAN - 1 for i in made) and any(i % F.SPAN == 0 for i in made), (period, sorted(made)[:8])
    assert set(F.period_targets(axis)) <= made and [t % F.SPAN for t in F.period_targets(axis)] == [0, F.SPAN - 1]
    lengths = {q[4] - q[3] for q in MM.quads_of(faces, MM.RUNS, True)}
    assert period in lengths and max(lengths) <= max(2 * period, 2), (period, sorted(lengths))
    if period == 7:
        floor("long_runs", "run heads at distinct item positions of a thread, period 7", len({i % 8 for i in made}))


# ---- checker -------------------------------------------------------------------------------------------------------------------------
def test_checker_has_a_group_of_equal_corners_across_a_block_boundary():
    for k, case in enumerate(F.checker()):
        cells = F.distinct(case.pos)
        assert len(cells) == F.CHECKER_SIDE ** 3 // 2 and not any(F.listed_neighbour(cells, o).any() for o in M.OFFSETS[:6])
        assert len(F.meshed("checker", k, MM.RUNS)[1]) == 12 * len(cells)                # every voxel has six exposed faces
        quads = MM.quads_of(MM.faces_of(source_of(case.pos, case.mrgb)), MM.RUNS, True)
        corners = sorted(c for q in quads for c in MM.corners_of(q))
        ends = [i for i in range(1, len(corners)) if corners[i] != corners[i - 1]]        # where a group begins
        begins = set(ends) | {0}
        straddled = [j for j in range(F.SPAN, len(corners), F.SPAN) if j not in begins]   # corners[j - 1] == corners[j]
        floor("checker", "groups of equal corner keys that straddle a block boundary", len(straddled))
        sizes = np.diff([0] + ends + [len(corners)])
        floor("checker", "entries of the longest group of equal corner keys", int(sizes.max()))


# ---- pairs ---------------------------------------------------------------------------------------------------------------------------
def test_pairs_are_what_they_claim():
    pairs = F.pairs()
    assert len(pairs) == 16
    kinds = [p.meta["kind"] for p in pairs]
    assert set(kinds) == {"moved", "subset", "superset", "bit 7", "one byte", "alternating"}
    for k, p in enumerate(pairs):
        kind = p.meta["kind"]
        a, b = source_of(*p.a), source_of(*p.b)
        if kind == "moved":
            step = [0, 0, 0]
            step[p.meta["axis"]] = (1, -1, 1)[p.meta["axis"]]
            assert {tuple(np.add(q, step).tolist()) for q in a} == set(b)
        if kind == "subset":
            assert set(b) < set(a) and len(F.combined(k, S.CHANGED)[0]) not in (0, len(b))
        if kind == "superset":
            assert set(a) < set(b)
        if kind == "bit 7":
            assert a == b and not np.array_equal(p.a[1], p.b[1]) and len(F.combined(k, S.CHANGED)[0]) == 0 == len(F.combined(k, S.CHANGED, True)[0])
        if kind == "one byte":
            # the changed byte sits at the merged index claimed (test_setops_cpu.test_the_straddle_lists_straddle)
            at, key = p.meta["at"], p.meta["key"]
            merged = F.merged_items(p.a[0], p.b[0])
            assert at in [F.SPAN * j - e for j in range(1, 5) for e in (0, 1)]
            assert merged[at][0] == key
            if at % 2:          # A's item closes a block and B's opens the next
                assert merged[at] == (key, 0) and merged[at + 1] == (key, 1) and (at + 1) % F.SPAN == 0
            else:               # A's item opens a block
                assert merged[at] == (key, 0) and merged[at + 1] == (key, 1) and at % F.SPAN == 0
            differ = [q for q in a if q in b and a[q] != b[q]]
            assert len(differ) == 1 and int(path_keys(np.array(differ, np.int64))[0]) == key
            assert F.combined(k, S.CHANGED)[0].tolist() == [list(differ[0])] and len(F.combined(k, S.CHANGED, True)[0]) == (1 if at % 2 == 0 else 2)
        if kind == "alternating":
            merged = F.merged_items(p.a[0], p.b[0])
            sides = [s for i, (key, s) in enumerate(merged) if not (i + 1 < len(merged) and merged[i + 1][0] == key) and not (i and merged[i - 1][0] == key)]
            runs = np.diff([0] + [i for i in range(1, len(sides)) if sides[i] != sides[i - 1]] + [len(sides)])
            assert runs.max() <= 9 + 9 and set(range(1, 10)) <= set(runs.tolist()) and set(a) & set(b)
        assert max(len(p.a[0]), len(p.b[0])) <= F.MAX_LIST and f"pairs[{k}]" in p.name and str(F.SEED) in p.name
    ats = sorted(p.meta["at"] for p in pairs if p.meta["kind"] == "one byte")
    assert ats == sorted(F.SPAN * j - e for j in range(1, 5) for e in (0, 1))


# ---- the rule programs ----------------------------------------------------------------------------------------------------------------
def words_of(mrgb):
    """morph_model.leaf_word of each row of a model's result (bit 7 of the material byte is clear there)"""
    return (0x80000000 | mrgb.astype(np.int64) @ np.array([1 << 24, 1 << 16, 1 << 8, 1])).tolist()


def keyed(result):
    pos, mrgb = result
    return list(zip(path_keys(pos.astype(np.int64)).tolist(), words_of(mrgb)))


CPU_MORPH_BARS = (0, 1, 2, 8, 11)          # of list_families.MORPH_BARS, which all run on the device


@pytest.mark.parametrize("fam", F.FAMILIES)
def test_the_morphologys_arithmetic_on_a_family(tmp_path, fam):
    exe = test_morph_cpu.build_rule_program(tmp_path)
    runs, want = [], []
    for k, case in enumerate(F.family(fam)):
        allowed = F.connectivities(fam, k)
        if not allowed or (fam == "long_runs" and k not in CPU_MORPH_BARS):
            continue
        c = allowed[k % len(allowed)]
        keys, words = M.sorted_keys_words(case.pos, case.mrgb)
        for op in (M.OPS if fam != "long_runs" else (M.OPS[k % 4], M.OPS[(k + 1) % 4])):      # a full bar: two ops, the model takes 10 s for four
            runs.append((keys, words, op, c, 1))
            want.append((k, keyed(F.morphed(fam, k, op, c))))
    assert len(runs) >= 6 and {r[2] for r in runs} == set(M.OPS)
    for (_, _, op, c, _), got, (k, exp) in zip(runs, test_morph_cpu.run_rule_program(exe, runs), want):
        assert got == exp, (fam, k, M.NAMES[op], c, len(got), len(exp))


@pytest.mark.parametrize("fam", F.FAMILIES)
def test_the_meshers_arithmetic_on_a_family(tmp_path, fam):
    exe = test_morph_cpu.build_rule_program(tmp_path, test_mesh_cpu.DRIVER)
    runs = []
    for k, case in enumerate(F.family(fam)):
        keys, words = M.sorted_keys_words(case.pos, case.mrgb)
        for mode in MM.MODES:
            if fam != "long_runs" or mode == MM.RUNS or k == 0:
                runs.append((k, mode, keys, words))
    results = test_mesh_cpu.run_rule_program(exe, [(mode, True, keys, words) for _, mode, keys, words in runs])
    for (k, mode, _, _), (verts, rows) in zip(runs, results):
        want = F.meshed(fam, k, mode)
        what = (fam, k, MM.NAMES[mode])
        assert (len(verts), len(rows)) == (len(want[0]), len(want[1])), what
        assert verts.tobytes() == want[0].tobytes() and np.array_equal(rows[:, :3], want[1]), what
        assert np.array_equal(rows[:, 3], np.array(words_of(want[2]))), what


def test_the_combiners_arithmetic_on_the_pairs(tmp_path):
    exe = test_morph_cpu.build_rule_program(tmp_path, test_setops_cpu.DRIVER)
    cases, want = [], []
    for k, p in enumerate(F.pairs()):
        lists = [S.sorted_keys_words(*p.a), S.sorted_keys_words(*p.b)]
        for swapped in (False, True):
            a, b = lists[::-1] if swapped else lists
            for op in S.OPS:
                cases.append((op, (*a, *b)))
                want.append(keyed(F.combined(k, op, swapped)))
    for n, (got, exp) in enumerate(zip(test_setops_cpu.run_rule_program(exe, cases), want)):
        assert got == exp, (n // 10, S.NAMES[n % 5], len(got), len(exp))
