"""The families of tests/transform_families.py are what they claim — checked with the models alone (no GPU, no library).  A family
that stopped landing on cell boundaries, stopped wrapping onto a listed voxel, or stopped putting a block's interval on the edge of
the source's bounding box would make the GPU comparison of tests/test_gpu_transform_families.py pass for nothing.  The model's
results are cached in transform_families and shared.  A claim that is a count or a share is held to transform_families.FLOOR."""
import numpy as np

import transform_families as F
import transform_model as T
from test_transform_cpu import build_rule_program, rule_program_agrees_with_the_model

ALL = [(fam, kind) for fam in F.FAMILIES for kind in F.KINDS]


def every_case():
    for fam, kind in ALL:
        for k in range(F.count(fam)):
            yield fam, kind, k, F.case(fam, kind, k)


# ---- the generators ----------------------------------------------------------------------------------------------------------------
def test_families_are_deterministic_and_within_their_sizes():
    total = 0
    for fam, kind, k, c in every_case():
        total += F.cells_of(c)
        assert 0 < F.cells_of(c) <= F.MAX_BOX, c.name
        assert c.pos.dtype == np.int16 and c.mrgb.dtype == np.uint8 and c.pos.shape == (len(c.mrgb), 3) and c.mrgb.shape[1] == 4, c.name
        assert fam in c.name and f"[{k}]" in c.name and kind in c.name and str(F.SEED) in c.name
        T.check_map(c.m, c.t)
        src = T.source_of(c.pos)
        assert len(src) < len(c.pos), f"{c.name}: some positions are listed twice"
    print(f"{total} cells in all")
    assert total <= F.MAX_TOTAL
    for fam in F.FAMILIES:
        assert 11 <= F.count(fam), fam
        assert [i for part in F.parts(fam) for i in part] == list(range(F.count(fam))), fam
    # drawn again from nothing, a case is the same bytes
    for fam in ("limits", "rigid", "near_miss", "ties"):
        before = F.case(fam, "from_map", 3)
        F.case.cache_clear(), F.specs.cache_clear()
        again = F.case(fam, "from_map", 3)
        assert before.pos.tobytes() == again.pos.tobytes() and before.mrgb.tobytes() == again.mrgb.tobytes(), fam
        assert (before.m, before.t, before.box_min, before.box_max) == (again.m, again.t, again.box_min, again.box_max), fam


def test_the_lists_are_what_they_claim():
    pos, _ = F.blob()
    assert F.bounds(pos) == ((-20, -20, -20), (19, 19, 19))
    lo, hi = F.bounds(F.far()[0])
    assert lo == (T.LO,) * 3 and hi == (T.HI,) * 3
    keys = F.path_keys(F.far()[0])
    assert int(keys.min()).bit_length() <= 8 and int(keys.max()).bit_length() == 48          # the keys use all 48 bits
    cl = np.unique(F.clustered()[0].astype(np.int64), axis=0)
    inside = ((cl >= np.array(F.CLUSTER_AT)) & (cl < np.array(F.CLUSTER_AT) + 16)).all(axis=1)
    print(f"clustered: {len(cl)} unique cells, {int(inside.sum())} in the cube")
    assert 4000 < len(cl) < 5000 and 0.88 < inside.mean() < 0.92 and np.abs(cl[~inside]).max() > 29000
    assert len(cl) > F.STAGED                                                                 # the search takes the sampled path
    lo, hi = F.bounds(F.line()[0])
    assert lo[:2] == hi[:2] and hi[2] - lo[2] > 2048
    lo, hi = F.bounds(F.plane()[0])
    assert lo[0] == hi[0] and hi[1] > lo[1] and hi[2] - lo[2] > 2048
    rng = np.random.default_rng(3)
    pts = rng.integers(-32768, 32768, (500, 3))
    assert F.path_keys(pts).tolist() == [T.path_key(p) for p in pts.tolist()]


def test_from_map_lists_hits_and_near_misses():
    missed = total = 0
    for fam in ("limits", "minify", "shear"):
        for k in range(F.count(fam)):
            c = F.case(fam, "from_map", k)
            want = F.expected(fam, "from_map", k)
            _, s, ok = F.pulled(c.m, c.t, F.box_cells(c.box_min, c.box_max))
            pulled = set(map(tuple, s[ok].tolist()))
            listed = set(T.source_of(c.pos))
            assert len(want[0]) >= len(listed & pulled) > 0 and len(listed - pulled) > 0, c.name
            missed, total = missed + len(listed - pulled), total + len(listed)
    print(f"from_map: {missed / total:.3f} of the listed voxels are pulled by no cell of their box")
    assert missed / total >= F.FLOOR["from_map", "share of listed voxels that no cell pulls"]


# ---- every case: the result, the models, the cull -----------------------------------------------------------------------------------
def test_every_result_is_neither_empty_nor_the_whole_box():
    for fam, kind, k, c in every_case():
        n, meta = len(F.expected(fam, kind, k)[0]), F.META[c.name]
        if meta.get("rank") == 0:
            assert n == (F.cells_of(c) if meta["whole"] else 0), c.name          # m = 0: all or nothing
        elif meta.get("empty"):
            assert n == 0, c.name                                                # the claim is emptiness
        else:
            assert 0 < n < F.cells_of(c), (c.name, n)
    for fam in ("singular", "past_range", "near_miss"):
        assert any(F.META[c.name].get("empty") or F.META[c.name].get("whole") is False for c in F.family(fam, "fixed")), fam


def test_the_python_loop_equals_the_numpy_walk_on_a_cut_of_every_case():
    for fam, kind, k, c in every_case():
        want = F.expected(fam, kind, k)
        mid = want[0][len(want[0]) // 2].astype(int).tolist() if len(want[0]) else list(F.middle_cell(c.box_min, c.box_max))
        lo = [max(int(a), v - e // 2) for a, v, e in zip(c.box_min, mid, (8, 12, 16))]           # 1 536 cells at most, about a voxel of the result
        hi = [min(int(b), v + e) for b, v, e in zip(c.box_max, lo, (8, 12, 16))]
        assert 0 < np.prod([b - a for a, b in zip(lo, hi)]) <= 3000
        loop, walk = T.transform(c.pos, c.mrgb, c.m, c.t, lo, hi), T.transform_np(c.pos, c.mrgb, c.m, c.t, lo, hi)
        assert np.array_equal(loop[0], walk[0]) and np.array_equal(loop[1], walk[1]), c.name
        inside = (want[0] >= np.array(lo)).all(axis=1) & (want[0] < np.array(hi)).all(axis=1)
        assert np.array_equal(want[0][inside], walk[0]) and np.array_equal(want[1][inside], walk[1]), c.name


def test_the_cull_drops_and_keeps_blocks_of_all_three_shapes_in_every_family():
    for fam in F.FAMILIES:
        dropped = kept = 0
        shapes = set()
        for kind in F.KINDS:
            for c in F.family(fam, kind):
                for shape, drop, _, _ in F.cull(c):
                    shapes.add(shape)
                    dropped, kept = dropped + drop, kept + (not drop)
        print(f"{fam}: {dropped} blocks dropped, {kept} kept, shapes {sorted(shapes)}")
        assert dropped > 0 and kept > 0, fam
        # rigid_box of a list is no z run of 2 048 cells unless the list is a rod (transform_families' docstring)
        assert shapes == ({"rows", "slab"} if fam == "rigid" else set(F.SHAPES)), (fam, shapes)
        assert any(min(c.box_min) == -32768 or max(c.box_max) == 32768 for c in F.family(fam, "fixed")), f"{fam}: a box clipped at the range"


def test_a_dropped_block_holds_no_voxel_of_the_result():
    """The restatement is the kernel's rule: what it drops must be what the model leaves empty, or the families prove nothing."""
    for fam, kind, k, c in every_case():
        want = F.expected(fam, kind, k)[0].astype(np.int64)
        ext = F.extents(c.box_min, c.box_max)
        rel = want - np.array(c.box_min)
        block_of = (rel[:, 0] * ext[1] * ext[2] + rel[:, 1] * ext[2] + rel[:, 2]) // F.SPAN
        drops = np.array([drop for _, drop, _, _ in F.cull(c)])
        assert not drops[block_of].any(), c.name


def test_near_miss_has_each_clearance_on_each_axis_side_and_block_shape():
    seen = set()
    for kind in F.KINDS:
        for c in F.family("near_miss", kind):
            meta = F.META[c.name]
            shape, axis, side, clear = meta["near"]
            got_shape, drop, below, above = F.cull(c)[meta["block"]]
            mine = (below if side == "below" else above)[axis]
            assert got_shape == shape and mine == clear, (c.name, got_shape, below, above)
            if clear == 1:
                assert drop and max(v for v in below + above if v is not mine) <= 0 or sum(v > 0 for v in below + above) == 1, c.name    # this axis alone drops it
            if clear == 0:
                assert not drop, c.name
            seen.add((kind, shape, axis, side, clear))
            assert all(abs(c.m[i][j]) == 0 for i in range(3) for j in range(3) if i != j)
    assert len(seen) == 2 * 3 * 3 * 2 * 3
    signs = {np.sign(c.m[i][i]) for c in F.family("near_miss", "fixed") for i in range(3)}
    sizes = {abs(c.m[i][i]) for c in F.family("near_miss", "fixed") for i in range(3)}
    assert signs == {1, -1} and len(sizes) >= 4 and F.ONE in sizes
    fixed = {F.META[c.name]["fixed"] for c in F.family("near_miss", "fixed")}
    assert fixed == {"blob", "plane", "line"}                     # bounding boxes that are a box, a plane and a line


# ---- family by family ---------------------------------------------------------------------------------------------------------------
def pulls(c):
    return F.pulled(c.m, c.t, F.box_cells(c.box_min, c.box_max))


def test_limits_reach_42_bits_with_every_entry_at_a_limit():
    bits = 0
    for kind in F.KINDS:
        for c in F.family("limits", kind):
            p, s, ok = pulls(c)
            bits = max(bits, int(np.abs(p).max()).bit_length(), int(np.abs(p - 2 * np.array(c.t)).max()).bit_length())
            assert any(abs(v) in (T.M_LIMIT, T.M_LIMIT - 1) for row in c.m for v in row), c.name
    print(f"limits: the greatest |P| or |sum m c| has {bits} bits")
    assert bits >= F.FLOOR["limits", "greatest |P| in bits"]
    cases = F.family("limits", "from_map")
    assert {abs(v) for c in cases for v in c.t} >= {T.T_LIMIT, T.T_LIMIT - 1}
    assert {v for c in cases for row in c.m for v in row} >= {T.M_LIMIT, -T.M_LIMIT, T.M_LIMIT - 1, 1 - T.M_LIMIT}
    # the six boxes where the sums cancel: every pulled cell in range, s within +-9 400, nearly every cell in the result
    for k in range(6):
        c = cases[k]
        p, s, ok = pulls(c)
        n = len(F.expected("limits", "from_map", k)[0])
        assert n > 2000 and ok.all() and np.abs(s).max() <= 9400 and F.cells_of(c) == 13824, c.name
        assert all(abs(v) >= T.T_LIMIT - 1 for v in c.t), c.name
    assert sum(np.linalg.matrix_rank(np.array(c.m, np.float64)) == 3 for c in cases) >= 4          # one row at the limits, rank 3


def test_magnify_fills_blocks_and_minify_hits_sparsely():
    full = 0
    for kind in F.KINDS:
        for k, c in enumerate(F.family("magnify", kind)):
            assert all(1 << 10 <= abs(c.m[i][i]) <= 1 << 15 for i in range(3)) and all(c.m[i][j] == 0 for i in range(3) for j in range(3) if i != j)
            want = F.expected("magnify", kind, k)[0].astype(np.int64)
            ext = F.extents(c.box_min, c.box_max)
            rel = want - np.array(c.box_min)
            per_block = np.bincount((rel[:, 0] * ext[1] * ext[2] + rel[:, 1] * ext[2] + rel[:, 2]) // F.SPAN, minlength=len(F.blocks(c.box_min, c.box_max)))
            full += int((per_block[:-1] == F.SPAN).sum()) + int(per_block[-1] == F.cells_of(c) - F.SPAN * (len(per_block) - 1))
    print(f"magnify: {full} blocks whose every cell hits")
    assert full >= F.FLOOR["magnify", "blocks whose every cell hits"]
    share = 0.0
    for kind in F.KINDS:
        for k, c in enumerate(F.family("minify", kind)):
            assert max(abs(v) for row in c.m for v in row) > 1 << 17, c.name
            share = max(share, len(F.expected("minify", kind, k)[0]) / F.cells_of(c))
    assert max(abs(v) for c in F.family("minify", "fixed") for row in c.m for v in row) > 1 << 23
    print(f"minify: at most {share:.3f} of a box hits")
    assert share <= F.FLOOR["minify", "greatest share of a box that hits"]


def test_shear_and_mirror_maps():
    for c in F.family("shear", "fixed"):
        assert all(c.m[i][i] == F.ONE for i in range(3)) and max(abs(c.m[i][j]) for i in range(3) for j in range(3) if i != j) <= 2 * F.ONE
    off = {c.m[i][j] for c in F.family("shear", "fixed") for i in range(3) for j in range(3) if i != j}
    assert 2 * F.ONE in off and -2 * F.ONE in off
    seen = set()
    for kind in F.KINDS:
        for k, c in enumerate(F.family("mirror", kind)):
            meta = F.META[c.name]
            assert round(float(np.linalg.det(np.array(meta["r"], np.float64)))) == -1 and len({v % 2 for v in meta["twice_pivot"]}) == 1, c.name
            _, s, ok = F.pulled(c.m, c.t, F.box_cells(c.box_min, c.box_max))
            assert ok.all() and len(np.unique(s, axis=0)) == F.cells_of(c), f"{c.name}: a bijection of the cells"
            seen.add(str(meta["r"]))
    assert len(seen) == 24
    assert {F.META[c.name]["twice_pivot"][0] % 2 for c in F.family("mirror", "fixed")} == {0, 1}


def test_ties_land_on_cell_boundaries_at_negative_coordinates():
    on, negative, differ, cells = 0, 0, 0, 0
    for kind in F.KINDS:
        for c in F.family("ties", kind):
            if F.META[c.name]["index"] < 12:
                assert all(a < 0 < b for a, b in zip(c.box_min, c.box_max)), c.name           # across 0 on every axis
            assert all(v % (F.ONE // 2) == 0 for row in c.m for v in row) and all(v % (F.ONE // 2) == 0 for v in c.t), c.name
            p, s, ok = pulls(c)
            on += int((p % (1 << 17) == 0).any(axis=1).sum())
            negative += int((p < 0).any(axis=1).sum())
            cells += len(p)
            differ += int(((p % (1 << 17) != 0) & (p < 0)).any(axis=1).sum())          # where a truncation is not the floor
    print(f"ties: P = 0 mod 2^17 on some axis for {on / cells:.3f} of the cells, P < 0 for {negative / cells:.3f}")
    assert on / cells >= F.FLOOR["ties", "share of cells with P = 0 mod 2^17 on some axis"]
    assert negative / cells >= F.FLOOR["ties", "share of cells with a negative P"]
    print(f"ties: a truncation differs from the floor on {differ / cells:.3f} of the cells")
    assert differ / cells >= F.FLOOR["ties", "share of cells where a truncation is not the floor"]
    assert any(v % F.ONE for c in F.family("ties", "fixed") for row in c.m for v in row)         # odd multiples of 32768 too


def wrapped(v, bits):
    return ((v + (1 << (bits - 1))) % (1 << bits)) - (1 << (bits - 1))


def test_past_range_cells_would_wrap_onto_listed_voxels_and_the_model_leaves_them_out():
    in16 = in32 = 0
    steps = set()
    for kind in F.KINDS:
        for k, c in enumerate(F.family("past_range", kind)):
            cells = F.box_cells(c.box_min, c.box_max)
            p, s, ok = F.pulled(c.m, c.t, cells)
            assert (~ok).any(), c.name
            listed = F.keys_of(np.asarray(c.pos, np.int64))
            s16 = wrapped(s, 16)
            hit16 = ~ok & np.isin(F.keys_of(s16), listed)
            s32 = wrapped(p, 32) >> 17
            hit32 = ~ok & ((s32 >= T.LO) & (s32 <= T.HI)).all(axis=1)
            hit32[hit32] = np.isin(F.keys_of(s32[hit32]), listed)
            in16, in32 = in16 + int(hit16.sum()), in32 + int(hit32.sum())
            assert hit16.any(), c.name
            got = set(map(tuple, F.expected("past_range", kind, k)[0].tolist()))
            assert not got & set(map(tuple, cells[hit16 | hit32].tolist())), c.name          # the model leaves every one of them out
            steps |= set(np.abs(s - s16)[~ok].max(axis=1).tolist())
            if F.META[c.name].get("empty"):
                assert not ok.any() and np.array_equal(s16[:, 0], cells[:, 0]) and hit16.sum() > 0, c.name
    print(f"past_range: {in16} cells wrap onto a listed voxel in 16 bits of s, {in32} in 32 bits of P")
    assert in16 >= F.FLOOR["past_range", "cells whose s wraps onto a listed voxel in 16 bits"]
    assert in32 >= F.FLOOR["past_range", "cells whose P wraps onto a listed voxel in 32 bits"]
    assert {1 << 16, 1 << 24} <= steps          # by one turn of 16 bits (1 to 3 cells, and exactly 2^16) and by 2^24 cells


def test_singular_maps_pull_one_voxel_from_many_cells():
    most = {0: 0, 1: 0, 2: 0}
    for kind in F.KINDS:
        for c in F.family("singular", kind):
            rank = F.META[c.name]["rank"]
            assert np.linalg.matrix_rank(np.array(c.m, np.float64)) == rank, c.name
            _, s, ok = pulls(c)
            _, counts = np.unique(s[ok], axis=0, return_counts=True)
            most[rank] = max(most[rank], int(counts.max()))
    print(f"singular: the most cells that pull one voxel, by rank: {most}")
    assert most[0] >= F.FLOOR["singular", "most cells that pull one voxel"]
    assert min(most[1], most[2]) >= F.FLOOR["singular", "most cells that pull one voxel, rank 1 and 2"]


def test_clustered_keys_fill_the_staged_sample_and_queries_land_between_clusters():
    cl = np.unique(F.clustered()[0].astype(np.int64), axis=0)
    keys = np.sort(F.path_keys(cl))
    cube_keys = F.path_keys(cl[((cl >= np.array(F.CLUSTER_AT)) & (cl < np.array(F.CLUSTER_AT) + 16)).all(axis=1)])
    sample = keys[(np.arange(F.STAGED) * len(keys)) >> 10]
    inside = int(np.isin(sample, cube_keys).sum())
    between = used = 0
    for fam in F.FAMILIES:
        for k, c in enumerate(F.family(fam, "fixed")):
            if F.META[c.name]["fixed"] != "clustered":
                continue
            used += 1
            _, s, ok = pulls(c)
            q = F.path_keys(s[ok])
            at = np.searchsorted(keys, q)
            miss = (at < len(keys)) & (at > 0) & (keys[np.minimum(at, len(keys) - 1)] != q)          # strictly between two listed keys
            between += int(miss.sum())
    print(f"clustered: {inside} of {F.STAGED} staged sample indices inside the cluster; {between} cells of {used} boxes pull a key between two clusters")
    assert inside >= F.FLOOR["clustered", "staged sample indices inside the cluster"]
    assert between >= F.FLOOR["clustered", "box cells whose key lies strictly between two clusters"]


def test_rigid_box_loses_no_cell_in_a_shell_three_cells_wide():
    from gpu_voxel_raytracer_amd import host as H

    def shell_is_clear(m, t, box, src_lo, src_hi, what):
        outer = tuple(max(-32768, v - 3) for v in box[0]), tuple(min(32768, v + 3) for v in box[1])
        cells = F.box_cells(*outer)
        cells = cells[~((cells >= np.array(box[0])) & (cells < np.array(box[1]))).all(axis=1)]
        _, s, ok = F.pulled(m, t, cells)
        into = ok & ((s >= np.array(src_lo)) & (s <= np.array(src_hi))).all(axis=1)
        assert len(cells) and not into.any(), what

    pivots = set()
    for c in F.family("rigid", "fixed"):
        meta = F.META[c.name]
        assert any(meta["shift"]), c.name
        shell_is_clear(c.m, c.t, (c.box_min, c.box_max), *F.bounds(c.pos), c.name)
        pivots.add(tuple(int(np.sign(v)) if abs(v) > 32000 else 0 for v in meta["pivot"]))
    assert len(pivots) == 9                                                        # the origin's neighbourhood and the eight corners
    assert sum(min(c.box_min) == -32768 or max(c.box_max) == 32768 for c in F.family("rigid", "fixed")) >= 8
    rng = np.random.default_rng([F.SEED, 9])
    for trial in range(300):                                                       # 12^3 cubes at the far corners
        corner = np.array(F.CORNERS[trial % 8])
        lo = np.clip(corner - np.sign(corner) * rng.integers(0, 40, 3) - 6, T.LO, T.HI - 11)
        r = F.random_rotation(rng)
        pivot = tuple((lo + 6 + (0.5 if trial % 2 else 0.0)).tolist())
        shift = tuple((rng.integers(-9, 10, 3) + 0.25 * rng.integers(0, 4, 3)).tolist())
        a = H.rigid_pull(r, pivot, shift)
        box = H.rigid_box(lo, lo + 11, r, pivot, shift)
        shell_is_clear([list(row) for row in a.m], list(a.t), box, lo, lo + 11, (trial, pivot, shift))


# ---- the shared arithmetic on the families' maps -------------------------------------------------------------------------------------
def test_the_kernels_arithmetic_on_the_families_under_the_sanitizers(tmp_path):
    """tests/test_transform_cpu.py's stand-alone program around csrc/transform_rule.h (g++ -fsanitize=undefined,address), fed about
    2 000 (m, t, d) triples of the families: its output equals the model's and the sanitizers report nothing."""
    exe = build_rule_program(tmp_path)
    rng = np.random.default_rng([F.SEED, 7])
    triples = []
    for fam in F.FAMILIES:
        for kind in F.KINDS:
            n = F.count(fam)
            per = max(2, 100 // n + 1)
            for k in range(n):
                c = F.case(fam, kind, k)
                corners = [(x, y, z) for x in (c.box_min[0], c.box_max[0] - 1) for y in (c.box_min[1], c.box_max[1] - 1) for z in (c.box_min[2], c.box_max[2] - 1)]
                picks = [corners[int(rng.integers(0, 8))]] + [tuple(int(rng.integers(a, b)) for a, b in zip(c.box_min, c.box_max)) for _ in range(per - 1)]
                triples += [(c.m, c.t, d) for d in picks]
    assert 1900 <= len(triples) <= 2600, len(triples)
    in_count = rule_program_agrees_with_the_model(exe, triples)
    assert 200 < in_count < len(triples) - 100                                  # both answers of the range test are exercised
