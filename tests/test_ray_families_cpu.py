"""The ray families of tests/ray_families.py are what they claim — checked with the oracle alone, on the scenes
tests/test_gpu_ray_walk.py sends them through (no GPU).  A family that stopped hitting anything, or stopped reaching one of the two
walks, would make the GPU comparison pass for nothing."""
import numpy as np
import pytest

import ray_families as R


@pytest.fixture(scope="module")
def cast(O, scenes):
    """scene -> {family: (origins, dirs, (hit, time, leaf, normal, trips))} from the oracle, computed once."""
    out = {}
    for name in R.SCENES:
        pos, mrgb = R.scene_voxels(name, scenes)
        octree = O.create_octree(pos, mrgb)
        fam = R.scene_families(name, pos, R.root_half_of(octree))
        out[name] = {k: (o, d, O.cast_rays(octree, o, d)) for k, (o, d) in fam.items()}
    return out


def test_families_are_deterministic_and_complete(O, scenes):
    pos, mrgb = R.scene_voxels("cube16")
    half = R.root_half_of(O.create_octree(pos, mrgb))
    assert half == 4.0
    a, b = R.scene_families("cube16", pos, half, n=500), R.scene_families("cube16", pos, half, n=500)
    assert tuple(a) == R.FAMILIES
    for k in a:
        for x, y in zip(a[k], b[k]):
            assert x.dtype == np.float32 and x.shape == (500, 3) and np.array_equal(x.view(np.uint32), y.view(np.uint32)), k
    assert "inside_solid" not in R.families(np.random.default_rng(1), [-0.5] * 3, [0.5] * 3, 0.5, 10)


def test_the_scenes_are_what_the_walk_tests_assume(O, scenes):
    depth = {name: O.voxel_depth(R.scene_voxels(name, scenes)[0]) for name in R.SCENES}
    assert depth == {"cube16": 3, "cube32": 4, "castle": 5, "one_voxel": 1, "empty": 0, "deep15": 15}
    for name, half in (("cube16", 8), ("cube32", 16)):
        pos, _ = R.scene_voxels(name)
        assert len(np.unique(pos, axis=0)) == len(pos)
        for axis in range(3):                      # touches every face of its root
            assert (pos[:, axis] == -half).any() and (pos[:, axis] == half - 1).any()
        assert len({tuple(p) for p in (pos >= 0).tolist()}) == 8     # all eight root slots occupied
    pos, _ = R.scene_voxels("castle", scenes)
    assert (pos >= 0).all()                        # one occupied root slot


def test_is_regular_restates_the_kernels_test():
    f = np.float32
    d = np.array([[1, 1, 1], [0, 1, 1], [1, -0.0, 1], [1, 1, np.nan], [np.inf, 1, 1], [1e-39, 1, 1], [3e-39, 1, 1], [3e38, 1, 1],
                  [1, 1e-45, 1], [-1, -1, -3.4e38]], f)
    # 1 / 1e-39 overflows, 1 / 3e-39 does not; 1 / 3e38 is subnormal but not zero
    assert R.is_regular(d).tolist() == [True, False, False, False, False, False, True, True, False, True]


def test_assert_rays_equal_sees_every_field():
    n = 4
    base = (np.array([1, 0, 1, 1], bool), np.array([0.0, 0.0, np.nan, 2.5], np.float32), np.array([-5, 0, -7, -9], np.int32),
            np.zeros((n, 3), np.float32))
    R.assert_rays_equal(base, tuple(a.copy() for a in base), "same")          # NaN time equals NaN time
    for field, index, value in ((0, 1, True), (1, 0, np.float32(-0.0)), (1, 1, np.float32(1.0)), (2, 3, -10), (3, (2, 1), np.float32(-0.0))):
        other = [a.copy() for a in base]
        other[field][index] = value
        with pytest.raises(AssertionError, match="1 of 4 rays differ"):
            R.assert_rays_equal(tuple(other), base, "changed", origins=np.zeros((n, 3), np.float32), dirs=np.ones((n, 3), np.float32))


def test_every_recorded_pair_reaches_its_hit_floor(cast):
    for (scene, family), floor in R.HIT_FLOOR.items():
        hits = int(cast[scene][family][2][0].sum())
        assert hits >= floor, (scene, family, hits, floor)
    for family in R.FAMILIES:            # every family hits somewhere (nonfinite_dir: only where the root's low faces hold voxels)
        assert any(f == family for _, f in R.HIT_FLOOR), family


def test_non_finite_rays_miss_where_nothing_lies_on_the_roots_low_faces(cast):
    for scene, family in R.ALL_MISS:
        hit, time = cast[scene][family][2][:2]
        assert not hit.any(), (scene, family, int(hit.sum()))
    # what hits elsewhere is a NaN in y or z alone: never an infinity, never a NaN in x
    for scene in ("cube16", "cube32"):
        o, d, res = cast[scene]["nonfinite_origin"]
        hit = res[0]
        assert not (np.isinf(o).any(1) | np.isnan(o[:, 0]))[hit].any()
        o, d, res = cast[scene]["nonfinite_dir"]
        hit = res[0]
        assert not (np.isinf(d).any(1) | np.isnan(d[:, 0]))[hit].any()


def test_every_family_reaches_the_walks_it_is_meant_for(cast):
    for scene in R.SCENES:
        for family, (o, d, _) in cast[scene].items():
            regular = int(R.is_regular(d).sum())
            least_regular, least_other = R.WALK_SPLIT[family]
            assert regular >= least_regular and len(d) - regular >= least_other, (scene, family, regular)
            if least_regular == 0:
                assert regular == 0
            if least_other == 0:
                assert regular == len(d)


def test_no_ray_reaches_the_trip_cap(cast):
    for scene in R.SCENES:
        for family, (o, d, res) in cast[scene].items():
            assert int(res[4].max()) < 2048, (scene, family)
            assert not (res[0] & (res[2] == np.int32(-2 ** 31))).any()


def test_inside_solid_starts_inside_a_voxel(cast):
    for scene in ("cube16", "cube32", "castle", "one_voxel", "deep15"):
        hit, time = cast[scene]["inside_solid"][2][:2]
        assert int((hit & (time == 0)).sum()) >= 14000, scene


@pytest.mark.parametrize("scene", ["cube16", "cube32"])
def test_a_nan_in_the_origins_x_is_a_miss_with_time_zero(cast, scene):
    """ray_cube_intersection (voxels.comp:73-90) takes max(max(en.x, en.y), en.z) by compare and select: a NaN in the FIRST operand
    stays, entry and exit are NaN and the root test fails — although the scene touches its root's low-x face, where a walk that
    dropped the NaN (fmax / fmin) would enter, go to the low-x side at every level and hit."""
    o, d, (hit, time, leaf, normal, trips) = cast[scene]["nonfinite_origin"]
    sharp = np.isnan(o[:, 0]) & R.is_regular(d)
    assert int(sharp.sum()) >= 1000
    assert not hit[sharp].any()
    assert (time[sharp].view(np.uint32) == 0).all() and (leaf[sharp] == 0).all() and (normal[sharp].view(np.uint32) == 0).all()
    # the same NaN in y or z alone is dropped, and such rays do hit
    dropped = ~np.isnan(o[:, 0]) & np.isnan(o[:, 1:]).any(1) & ~np.isinf(o).any(1)
    assert int(hit[dropped].sum()) >= 1000


def test_the_issues_minimal_case(O):
    """One voxel at (-1, 0, 0), origin (NaN, 0.25, -5), direction normalize(0.01, 0.01, 1): a miss with time 0."""
    octree = O.create_octree(np.array([[-1, 0, 0]], np.int16), np.array([[0, 10, 20, 30]], np.uint8))
    d = np.array([[0.01, 0.01, 1.0]], np.float64)
    d = (d / np.linalg.norm(d)).astype(np.float32)
    hit, time, leaf, normal, _ = O.cast_rays(octree, np.array([[np.nan, 0.25, -5]], np.float32), d)
    assert not hit[0] and time.view(np.uint32)[0] == 0 and leaf[0] == 0
    hit, time, leaf, normal, _ = O.cast_rays(octree, np.array([[-0.25, 0.25, -5]], np.float32), d)      # the voxel is there
    assert hit[0] and abs(float(time[0]) - 5.0005) < 1e-3
