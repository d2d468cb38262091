"""GPU: vxrt_transform_voxels_device on the families of tests/transform_families.py — maps at the header's limits, magnifying,
minifying, shearing, singular and mirroring maps, pulls that land on cell boundaries at negative coordinates, pulls past the int16
range that would wrap onto a listed voxel, rigid motions at the corners of the range, and diagonal maps placed so that a block's
interval ends one cell short of, on, and one cell inside the source's bounding box — against lists made from the map itself, a
clustered list, lists whose bounding box is a line or a plane, and a list at the eight corners of the range.

Every case goes through test_gpu_transform.check, imported and not copied: exact positions and bytes against the model's walk of the
whole box (transform_families.expected), guard bytes, untouched inputs, a second call writing the same bytes, the count-only form
and the wrapper with and without cap.  On top of that the mirrors are taken back to the source, rotate_voxels is held equal to the
direct call into rigid_box, and each family has a case at odd addresses and a case without mrgb.  Every message carries the family,
the case's index and the seed (Case.name).  tests/test_transform_families_cpu.py holds each family to be what it claims.

What notices what (MI355X; each one-line mutation applied to a scratch copy of csrc, built as an A/B library through
_build.build(extra_flags=..., out=...) and selected with VXRT_LIB; this file's 84 cases and the 19 of tests/test_gpu_transform.py run
once against each; none of the mutated sources is kept).  Every mutation keeps each index inside [0, count) and every loop bound.

| # | mutation | test_gpu_transform.py fails | this file fails | the cases here that notice |
|---|---|---|---|---|
| 1 | `p >> 17` -> `p / 131072` (transform_rule.h) | 17 of 19 | 81 of 84 | every part but ties-fixed-2 and the all-out-of-range parts past_range-*-1 |
| 2 | the range test after narrowing s to int16_t | 1 (test_a_pull_past_the_range_is_absent_not_wrapped) | 4 | past_range-from_map-0 and -2, past_range-fixed-0 and -2 |
| 3 | `2 d + 1` -> `2 d` in pull_cell | 10 | 79 | all but ties-from_map-2 and past_range-*-0 / -1 |
| 4 | the cull's `<` -> `<=` | 9 | 40 | all 18 parts of near_miss, 12 of mirror, 4 of singular, ties-fixed-0 to -2, magnify-from_map-0 and -1, one of shear-fixed |
| 5 | the cull's `>` -> `>=` | 9 | 42 | all 18 parts of near_miss, 13 of mirror, 5 of singular, ties-fixed-0 to -2, magnify-from_map-0 and -1, one of shear-fixed |
| 6 | the cull's box always [p, q] per axis | 10 | 47 | 14 parts of near_miss, 16 of mirror, all 8 of rigid, limits-fixed-0 and -1, minify-fixed-0 and -1, shear-fixed-0 and -1, 2 of singular-fixed, one of ties-fixed |
| 7 | `sample[...] <= key` -> `<` | 17 | 81 | every part but limits-fixed-0 and past_range-*-1 |
| 8 | `v[j] <= key[j]` -> `<` | 14 | 75 | every family in both kinds; 7 parts of from_map lists of at most 1 024 keys, which take no step in global memory, and past_range-*-1 pass |

Mutation 2 with int32_t instead of int16_t was not built: |s| < 2^26 under the header's limits, so it cannot change a result
(transform_families' docstring).  The hand-written file already noticed each of the eight; what the families add is the named
place — the one-cell clearances of near_miss for 4 to 6, past_range's wraps for 2 — and the maps the table above had never run.
The -DVXRT_TRANSFORM_NO_SAMPLE library passes both files as the product does (103 of 103).
"""
import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import transform_families as F
import transform_model as T
from test_gpu_transform import check, ctx, on_device  # noqa: F401  (ctx is the module's context fixture)

pytestmark = pytest.mark.gpu


ODD, BARE = 1, 2          # the family's case that is run again at odd addresses (from_map) and without mrgb (fixed)
PARTS = [(fam, kind, part) for fam in F.FAMILIES for kind in F.KINDS for part in range(len(F.parts(fam)))]


def back_through_the_mirror(H, ctx, case, there):
    """The inverse mirror of a result returns, in path order, the source voxels that the box pulled."""
    meta = F.META[case.name]
    r, twice_pivot = meta["r"], meta["twice_pivot"]
    src = T.source_of(case.pos, case.mrgb)
    _, s, ok = F.pulled(case.m, case.t, there[0].astype(np.int64))
    assert ok.all(), case.name
    keys = sorted({tuple(v) for v in s.tolist()}, key=T.path_key)
    assert len(keys) == len(there[0]), f"{case.name}: a mirror is a bijection of the cells"
    want = np.array(keys, np.int16).reshape(-1, 3), np.array([src[k] for k in keys], np.uint8).reshape(-1, 4)
    inverse = [[r[j][i] for j in range(3)] for i in range(3)]
    lo, hi = F.bounds(want[0])
    box = tuple(v - 1 for v in lo), tuple(v + 2 for v in hi)
    check(H, ctx, there[0], there[1], *T.rotation_pull(inverse, twice_pivot), *box, f"{case.name}: and back", want=want)


@pytest.mark.parametrize("fam,kind,part", PARTS, ids=[f"{f}-{k}-{p}" for f, k, p in PARTS])
def test_family(H, ctx, fam, kind, part):
    for k in F.parts(fam)[part]:
        case = F.case(fam, kind, k)
        want = F.expected(fam, kind, k)
        meta = F.META[case.name]
        got = check(H, ctx, case.pos, case.mrgb, case.m, case.t, case.box_min, case.box_max, case.name, want=want)
        if fam == "mirror" and len(got[0]):
            back_through_the_mirror(H, ctx, case, got)
        if fam == "rigid":
            w_pos, w_mrgb = ctx.rotate_voxels(on_device(case.pos), on_device(case.mrgb), meta["rotation"], meta["pivot"], meta["shift"])
            assert np.array_equal(w_pos.cpu().numpy(), got[0]) and np.array_equal(w_mrgb.cpu().numpy(), got[1]), f"{case.name}: rotate_voxels"
        if kind == "from_map" and k == ODD:
            check(H, ctx, case.pos, case.mrgb, case.m, case.t, case.box_min, case.box_max, f"{case.name}: addresses = 3 mod 16", want=want, shift=3)
        if kind == "fixed" and k == BARE:
            check(H, ctx, case.pos, None, case.m, case.t, case.box_min, case.box_max, f"{case.name}: positions only", want=(want[0], None))
