"""GPU: vxrt_combine_voxels_device, vxrt_morph_voxels_device and vxrt_mesh_voxels_device on the families of tests/list_families.py —
clusters across every seam +-2^k of the interleaved keys, patches on the faces, edges and corners of the int16 range, cells uniform
over the whole range, lists whose distinct count stands at 2^k - 1, 2^k, 2^k + 1 and at the block's multiples, meshes whose vertex
count does, bars of the full 65 536 cells in one colour, in periods that put run heads on both sides of a block and in colours that
differ in bit 7 alone, the checkerboard, and pairs of such lists for the combiner.

Every case goes through the hand-written files' ladders, imported and not copied (test_gpu_setops.check, test_gpu_morph.check,
test_gpu_mesh.check): exact positions, bytes, order and counts against the model (list_families.morphed / meshed / combined, computed
once per case), guard bytes, untouched inputs, a second call writing the same bytes, the count-only form, the wrapper with and
without a cap, and for a mesh without a coordinate of 32767 the way back through the solid voxeliser.  Morphology: all four ops at
each connectivity the case is allowed (list_families.connectivities); mesh: both modes, with and without bytes; combine: all five
ops, both ways round.  Per family one case runs again at addresses 3 mod 16, one with positions only, one two steps deep, and seams,
range_faces and sizes once through the tile lookup.  On top, identities between the operators on the device alone
(test_the_operators_agree_with_each_other, test_volumes_of_a_pairs_union_and_intersection).  Every message carries the family, the
case's index and the seed.  tests/test_list_families_cpu.py holds each family to be what it claims.

A part is sized by what its model costs (PART_CELL_ROWS, PART_FACES); a list over that is a part of its own, and a full bar one
part per op or mode.  205 cases, 225 s in all on an MI355X machine, the models included.
The slowest ids of `pytest --durations=15` there: long_runs-identities 3.9 s, far-mesh-1 3.0 s, long_runs-mesh-28 3.0 s,
long_runs-mesh-26, -12 and -18 2.8 s, far-mesh-0 2.8 s, long_runs-mesh-24, -16, -20, -14, -30, -32 and -22 2.6 to 2.7 s,
sizes-mesh-2 2.6 s.  The figures move by some tenths of a second from run to run; no id is well beyond the others.

What notices what (MI355X; each one-line mutation applied to a scratch copy of csrc, built as an A/B library through
_build.build(extra_flags=..., out=...) and selected as VXRT_LIB does; this file's 205 cases and the 75 of tests/test_gpu_setops.py,
tests/test_gpu_morph.py and tests/test_gpu_mesh.py run once against each; none of the mutated sources or libraries is kept).  Every
mutation keeps each index inside its array and every loop bound: each changes a value that is compared, sorted or written, never
an index or a trip count, and the counting and the writing pass of a kernel share the changed code.  The product library passes
both sets (280 of 280).  The last column counts this file's failing cases by family.  (The runs predate the two-step dilation of
the bar's piece inside long_runs-morph-extras, an id that mutations 1 and 11 fail without it.)

| # | mutation | hand-written files fail | this file fails | the cases here that notice |
|---|---|---|---|---|
| 1 | `(part | fill) + add` -> `part + add` in step_axis (morph_rule.h) | 50 (13 mesh, 37 morph) | 129 | checker 7, far 12, long_runs 19, pairs 2, range_faces 6, seams 13, sizes 53, vertex_counts 17 |
| 2 | `edge` of step_axis for d < 0 made unreachable: -1 wraps at 0 (morph_rule.h) | 5 (1 mesh, 4 morph) | 44 | far 2, long_runs 36, range_faces 6 |
| 3 | rows_of(c) one row short (morph_rule.h) | 36 (36 morph) | 89 | checker 7, far 7, long_runs 12, range_faces 3, seams 10, sizes 37, vertex_counts 13 |
| 4 | mesh_is_head without its `!= 0xffff` term (mesh_rule.h) | 1 (test_the_ends_of_the_int16_range) | 1 | range_faces-mesh-0 |
| 5 | mesh_corner_pack with 16-bit fields (mesh_rule.h) | 13 (13 mesh) | 70 | checker 3, far 5, long_runs 36, range_faces 3, seams 3, sizes 16, vertex_counts 4 |
| 6 | `0x1ffff` -> `0xffff` for z in mesh_corner_vertex (mesh_rule.h) | 1 (test_the_ends_of_the_int16_range) | 15 | far 2, long_runs 10, range_faces 3 |
| 7 | `c1 = q.c + len` taken mod 65 536 (mesh_rule.h) | 1 (test_the_ends_of_the_int16_range) | 41 | far 2, long_runs 36, range_faces 3 |
| 8 | `before` taken from `at` in mesh_heads_kernel (mesh.hip) | 13 (13 mesh) | 35 | far 2, long_runs 18, range_faces 1, seams 1, sizes 11, vertex_counts 2 |
| 9 | merge_corank's tie the other way, `<=` -> `<` (setops_rule.h) | 38 (27 morph, 11 setops) | 82 | checker 7, far 5, pairs 13, range_faces 3, seams 10, sizes 31, vertex_counts 13 |
| 10 | kSetopNoKey staged for the one key past the tile's B range (setops.hip) | 21 (18 morph, 3 setops) | 54 | checker 6, far 4, pairs 6, range_faces 1, seams 6, sizes 22, vertex_counts 9 |
| 11 | merge_takes_a compares the keys' low 32 bits (setops_rule.h) | 47 (27 morph, 20 setops) | 112 | checker 8, far 8, long_runs 8, pairs 21, range_faces 4, seams 11, sizes 38, vertex_counts 14 |
| 12 | walk_take's `probed <= q` -> `<` (morph_rule.h) | 44 (14 mesh, 30 morph) | 142 | checker 8, far 10, long_runs 39, pairs 2, range_faces 6, seams 13, sizes 47, vertex_counts 17 |
| 13 | mesh_coord drops bit 15 of u (mesh_rule.h) | 14 (14 mesh) | 69 | checker 2, far 4, long_runs 36, pairs 1, range_faces 3, seams 3, sizes 16, vertex_counts 4 |
| 14 | opposite_row of rows 18 to 25 is the row itself (morph_rule.h) | 7 (7 morph) | 29 | checker 2, far 2, range_faces 3, seams 5, sizes 17 |

The hand-written files already noticed each of the fourteen; none passes both sets, so no case had to be added for one.  What
the families add is where it is noticed.  2, 6 and 7 (a coordinate of 0 or 65 536) failed one or five hand-written tests, the
voxels at the ends of the range, and fail here on every full bar, the patches of range_faces and far's cells at 32767; 4 is
noticed only where a row's last cell (c = 65535) is followed by the next row's first: test_the_ends_of_the_int16_range there, the
patch on the range's edge in range_faces-mesh-0 here, and no bar can notice it (a bar's run ends with its row).  8 (every face
a head) is noticed by the RUNS part of the bars of every axis and colouring.  10 (the key past the tile) is noticed by the
combiner only where an equal pair lies across two blocks (3 hand-written tests; here pairs-combine-3, the subset over the whole
range, the four one-byte pairs at 2048 j - 1, pairs-combine-6, -8, -10 and -12, and pairs-volumes-6) and otherwise through
DILATE's merge.  14 (a wrong first source among the corner
neighbours) changes bytes alone and only at 26.
Not built: `i == 0u` dropped from run_is_head (morph_rule.h), the test behind the distinct corners.  The load in front of entry 0
is clamped to the array's last entry, and the sorted corner keys of a mesh that is not empty hold at least 8 distinct values, so
first and last always differ: no mesh notices it.  tests/test_gpu_run_heads.py does, with one key and with equal keys.  Nor tile_decides' `<=` -> `<`: a key equal to the tile's last is then asked of the whole array,
which answers the same.
"""
import ctypes as C

import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import list_families as F
import mesh_model as MM
import morph_model as M
import setops_model as S
from list_op_harness import on_device
from test_gpu_mesh import check as check_mesh
from test_gpu_morph import check as check_morph, ctx  # noqa: F401  (ctx is the module's context fixture)
from test_gpu_setops import check as check_combine

pytestmark = pytest.mark.gpu

PART_CELL_ROWS = 60_000          # distinct cells times connectivity per morphology part: 3 s per id at the most on an MI355X machine, the model included
PART_FACES = 12_000              # distinct cells per mesh part: 3 s per id at the most there
ODD = 3                          # addresses 3 mod 16
# the case of each family that runs again at odd addresses, with positions only and through the identities, and the connectivity
EXTRA = {"seams": (1, 18), "range_faces": (1, 26), "far": (0, 6), "sizes": (F.size_counts().index(F.SPAN + 1), 26),
         "vertex_counts": (F.vertex_reachable().index(2049), 18), "long_runs": (0, 6), "checker": (1, 6)}
# ... and the case and connectivity that run two steps deep: the second step's model works on the first's result, 7 to 27 times the list
TWO_STEPS = {"seams": (1, 6), "range_faces": (1, 18), "far": (2, 6), "sizes": (F.size_counts().index(129), 18),
             "vertex_counts": (F.vertex_reachable().index(2049), 6), "long_runs": (0, 6), "checker": (1, 6)}


def cells_of(fam, k):
    return len(F.distinct(F.case(fam, k).pos))


def _morph_parts():
    """-> [(family, [(case, connectivity, ops)])]"""
    parts = []
    for fam in F.FAMILIES:
        open_part, weight = [], 0
        for k in range(len(F.family(fam))):
            for c in F.connectivities(fam, k):
                w = cells_of(fam, k) * c
                if fam == "long_runs":
                    parts += [(fam, [(k, c, (op,))]) for op in M.OPS]
                elif w > PART_CELL_ROWS:
                    parts += [(fam, [(k, c, M.OPS[:2])]), (fam, [(k, c, M.OPS[2:])])] if w > 1.5 * PART_CELL_ROWS else [(fam, [(k, c, M.OPS)])]
                else:
                    if weight + w > PART_CELL_ROWS:
                        parts.append((fam, open_part))
                        open_part, weight = [], 0
                    open_part.append((k, c, M.OPS))
                    weight += w
        if open_part:
            parts.append((fam, open_part))
    return parts


def _mesh_parts():
    """-> [(family, [(case, mode, bare)])]"""
    parts = []
    for fam in F.FAMILIES:
        open_part, weight = [], 0
        for k in range(len(F.family(fam))):
            if fam == "long_runs":
                parts += [(fam, [(k, mode, False)]) for mode in MM.MODES]
                parts += [(fam, [(k, mode, True)]) for mode in MM.MODES if k < 3]          # without bytes a bar is its axis
                continue
            w = cells_of(fam, k)
            every = [(k, mode, bare) for mode in MM.MODES for bare in (False, True)]
            if w > PART_FACES:
                parts += [(fam, every[:2]), (fam, every[2:])]
            else:
                if weight + w > PART_FACES:
                    parts.append((fam, open_part))
                    open_part, weight = [], 0
                open_part += every
                weight += w
        if open_part:
            parts.append((fam, open_part))
    return parts


def _ids(parts, operator):
    seen, ids = {}, []
    for fam, _ in parts:
        ids.append(f"{fam}-{operator}-{seen.get(fam, 0)}")
        seen[fam] = seen.get(fam, 0) + 1
    return ids


MORPH_PARTS, MESH_PARTS = _morph_parts(), _mesh_parts()


# ---- the ladders -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,runs", MORPH_PARTS, ids=_ids(MORPH_PARTS, "morph"))
def test_morph(H, ctx, fam, runs):
    for k, c, ops in runs:
        case = F.case(fam, k)
        for op in ops:
            check_morph(ctx, case.pos, case.mrgb, op, c, 1, case.name, want=F.morphed(fam, k, op, c))


@pytest.mark.parametrize("fam", F.FAMILIES, ids=[f"{fam}-morph-extras" for fam in F.FAMILIES])
def test_morph_at_odd_addresses_positions_only_and_two_steps_deep(H, ctx, fam):
    k, c = EXTRA[fam]
    case = F.case(fam, k)
    assert c in F.connectivities(fam, k)
    check_morph(ctx, case.pos, case.mrgb, M.DILATE, c, 1, f"{case.name}: addresses = {ODD} mod 16", shift=ODD, want=F.morphed(fam, k, M.DILATE, c))
    check_morph(ctx, case.pos, None, M.SURFACE, c, 1, f"{case.name}: positions only", want=F.morphed(fam, k, M.SURFACE, c, 1, True))
    k, c = TWO_STEPS[fam]
    case = F.case(fam, k)
    assert c in F.connectivities(fam, k)
    # two steps of a full bar's dilation are 850 000 cells in the model: the bar erodes, which the first step ends, and a piece
    # of 4 097 cells of a coloured bar dilates, so that the second step's offers and merge work on the first's result
    for op in ((M.ERODE, M.SURFACE) if fam == "long_runs" else M.OPS):
        check_morph(ctx, case.pos, case.mrgb, op, c, 2, case.name, want=F.morphed(fam, k, op, c, 2))
    if fam == "long_runs":
        piece = F.bar_piece()
        for op in (M.DILATE, M.MARGIN):
            check_morph(ctx, piece.pos, piece.mrgb, op, c, 2, piece.name, want=F.morphed_piece(op, c, 2))


@pytest.mark.parametrize("fam", ["seams", "range_faces", "sizes"], ids=lambda fam: f"{fam}-morph-tile")
def test_morph_through_the_tile_lookup(H, ctx, fam):
    # morph_mask_kernel<true> (vxrt_debug.h), as test_gpu_morph.test_the_tile_lookup_gives_the_same_bytes runs it
    k, _ = EXTRA[fam]
    case = F.case(fam, k)
    assert ctx._L.vxrt_debug_morph_tile_lookup(ctx._h, C.c_uint32(1)) == 0
    try:
        for c in F.connectivities(fam, k):
            for op in M.OPS:
                check_morph(ctx, case.pos, case.mrgb, op, c, 1, f"{case.name}: tile lookup", want=F.morphed(fam, k, op, c))
    finally:
        assert ctx._L.vxrt_debug_morph_tile_lookup(ctx._h, C.c_uint32(0)) == 0


@pytest.mark.parametrize("fam,runs", MESH_PARTS, ids=_ids(MESH_PARTS, "mesh"))
def test_mesh(H, ctx, fam, runs):
    for k, mode, bare in runs:
        case = F.case(fam, k)
        check_mesh(ctx, case.pos, None if bare else case.mrgb, mode, case.name + (": positions only" if bare else ""), want=F.meshed(fam, k, mode, bare))


@pytest.mark.parametrize("fam", F.FAMILIES, ids=[f"{fam}-mesh-extras" for fam in F.FAMILIES])
def test_mesh_at_odd_addresses(H, ctx, fam):
    k, _ = EXTRA[fam]
    case = F.case(fam, k)
    check_mesh(ctx, case.pos, case.mrgb, MM.RUNS, f"{case.name}: addresses = {ODD} mod 16", shift=ODD, want=F.meshed(fam, k, MM.RUNS))


PAIRS = list(range(len(F.pairs())))


@pytest.mark.parametrize("k", PAIRS, ids=[f"pairs-combine-{k}" for k in PAIRS])
def test_combine(H, ctx, k):
    pair = F.pairs()[k]
    for swapped in (False, True):
        a, b = (pair.b, pair.a) if swapped else (pair.a, pair.b)
        for op in S.OPS:
            check_combine(ctx, *a, *b, op, pair.name + (": B with A" if swapped else ""), want=F.combined(k, op, swapped))


def test_combine_at_odd_addresses_and_positions_only(H, ctx):
    odd, bare = 0, F.pairs().index(next(p for p in F.pairs() if p.meta["kind"] == "alternating"))
    pair = F.pairs()[odd]
    for op in S.OPS:
        check_combine(ctx, *pair.a, *pair.b, op, f"{pair.name}: addresses = {ODD} mod 16", shift=ODD, want=F.combined(odd, op))
    pair = F.pairs()[bare]
    for op in (S.UNION, S.INTERSECT, S.DIFFERENCE, S.XOR):
        check_combine(ctx, pair.a[0], None, pair.b[0], None, op, f"{pair.name}: positions only", want=F.combined(bare, op, False, True))


# ---- identities between the operators, on the device alone -----------------------------------------------------------------------
@pytest.mark.parametrize("fam", F.FAMILIES, ids=[f"{fam}-identities" for fam in F.FAMILIES])
def test_the_operators_agree_with_each_other(H, ctx, fam):
    k, _ = EXTRA[fam]
    case = F.case(fam, k)
    d_pos, d_mrgb = on_device(case.pos), on_device(case.mrgb)
    for c in F.connectivities(fam, k):
        eroded = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_ERODE, c)
        surface = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_SURFACE, c)
        want = ctx.combine_voxels(d_pos, d_mrgb, eroded[0], None, H.LIST_DIFFERENCE)
        assert len(surface[0]) > 0 and torch.equal(surface[0], want[0]) and torch.equal(surface[1], want[1]), (case.name, c, "SURFACE")
        dilated = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_DILATE, c)
        margin = ctx.morph_voxels(d_pos, d_mrgb, H.MORPH_MARGIN, c)
        want = ctx.combine_voxels(*dilated, d_pos, None, H.LIST_DIFFERENCE)
        assert len(margin[0]) > 0 and torch.equal(margin[0], want[0]) and torch.equal(margin[1], want[1]), (case.name, c, "MARGIN")
    m = cells_of(fam, k)
    for mode in (H.MESH_FACES, H.MESH_RUNS):
        verts, tris, _ = ctx.mesh_voxels(d_pos, d_mrgb, mode)
        assert MM.volume6(verts.cpu().numpy(), tris.cpu().numpy()) == 6 * m, (case.name, mode)
        if mode == H.MESH_FACES:
            assert not any(n % 2 for n in MM.edge_counts(tris.cpu().numpy()).values()), case.name


VOLUME_PAIRS = [next(k for k, p in enumerate(F.pairs()) if p.meta["kind"] == kind) for kind in ("moved", "superset", "one byte", "alternating")]


@pytest.mark.parametrize("k", VOLUME_PAIRS, ids=[f"pairs-volumes-{k}" for k in VOLUME_PAIRS])
def test_volumes_of_a_pairs_union_and_intersection(H, ctx, k):
    pair = F.pairs()[k]
    dev = [on_device(v) for v in (*pair.a, *pair.b)]

    def volume(pos, mrgb):
        verts, tris, _ = ctx.mesh_voxels(pos, mrgb, H.MESH_RUNS)
        return MM.volume6(verts.cpu().numpy(), tris.cpu().numpy())

    union, both = ctx.combine_voxels(*dev, H.LIST_UNION), ctx.combine_voxels(*dev, H.LIST_INTERSECT)
    assert len(both[0]) > 0 or pair.meta["kind"] == "moved"
    assert volume(*union) + volume(*both) == volume(dev[0], dev[1]) + volume(dev[2], dev[3]), pair.name
