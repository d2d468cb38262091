"""The oracle's temporal stage (O.temporal: shaders/temporal.comp:48-125) against temporal_f64, a float64 restatement written from the
shader's text (tests/temporal_model.py), on synthetic history under camera motion.  The oracle binds texture() and inverse() to its own
sampler and affine inverse (U4 / U5); the only other restatement of the stage (test_oracle_shading_independent.py) covers a camera at
rest, where neither matters.  Here both are checked under every kind of motion, with exotic pixels in both frames."""
import numpy as np
import pytest

import temporal_model as M

# (sample_blending, maximum_blending, blending_distance_cutoff): the defaults and corners of the GUI's ranges (all on [0, 1])
PARAMS = [(0.5, 0.98, 1e-2), (0.25, 0.5, 1.0), (0.0, 0.98, 1e-2), (1.0, 1.0, 1e-2), (0.5, 0.0, 1e-4), (0.5, 0.98, 0.0)]


@pytest.mark.parametrize("w,h", [(96, 72), (65, 67)])
@pytest.mark.parametrize("motion", M.MOTIONS)
def test_oracle_temporal_equals_the_float64_model_under_motion(O, motion, w, h):
    f = M.synthetic_frames(O, w, h, motion, seed=w * 31 + M.MOTIONS.index(motion))
    args = (f["color"], f["nd"], f["old_color"], f["old_nd"], f["cam"], f["old_cam"])
    for p in PARAMS:
        tu = O.Temporal(*p)
        got = O.temporal(*args, tu, True)
        ref = M.temporal_f64(*args, tu)
        bad = M.disagreement(got, ref)
        assert not bad.any(), f"{motion}, params {p}: {int(bad.sum())} pixels differ; first {tuple(np.argwhere(bad)[0])}"
        assert ref["fragile"].mean() <= 0.05, (motion, p, ref["fragile"].mean())
        comparable = ~ref["fragile"] & ref["cmp_rgb"] & ref["cmp_a"]
        assert comparable.mean() > 0.9
        if p[2] == 0.0:
            assert not ref["accepted"].any()                    # dist < 0 is never true
    # coverage at the default parameters and at the widest cutoff
    ref = M.temporal_f64(*args, O.Temporal(*PARAMS[0]))
    wide = M.temporal_f64(*args, O.Temporal(*PARAMS[1]))
    hit = ~ref["sky"]
    for k in ("sky", "outside", "rejected", "accepted"):
        assert ref[k].any(), (motion, k)
    accepted = wide["accepted"].sum() / hit.sum()
    if motion == "out_of_view":
        assert ref["outside"].sum() > 0.4 * hit.sum()
    else:
        assert accepted >= 0.3, (motion, accepted)
    if motion == "behind":
        assert ref["behind"].sum() >= 10
    if motion in ("rest", "pixel_pan"):                         # reprojections on texel centres: weights exactly 0 or 1
        assert wide["edge"].sum() > 0.2 * wide["accepted"].sum()
    else:
        assert wide["edge"].sum() < 0.5 * wide["accepted"].sum()
    if motion == "drift":
        assert wide["edge"].any()
    # exotic history actually reaches accepted pixels: NaN / inf colours and off-ladder factors
    reached = wide["accepted"] & (~wide["cmp_rgb"] | ~wide["cmp_a"] | np.isnan(wide["rgb"]).any(-1))
    assert reached.any() or motion == "out_of_view", motion


def test_zero_weight_texels_are_not_read(O):
    """A NaN texel beside a reprojection that lands on a texel centre: its weight is exactly 0, so it must not leak in (the
    project's rule, oracle U4); a reprojection half a texel away gives it weight 1/2, and it must."""
    w, h = 64, 48
    f = M.synthetic_frames(O, w, h, "rest", seed=7, exotic=False)
    args = [f["color"], f["nd"], f["old_color"].copy(), f["old_nd"], f["cam"], f["old_cam"]]
    args[2][::2, ::2, :3] = np.nan                              # every other texel in both directions
    tu = O.Temporal.default()
    got = O.temporal(*args, tu, True)
    ref = M.temporal_f64(*args, tu)
    assert ref["edge"].sum() == ref["accepted"].sum() > 0.5 * (~ref["sky"]).sum()
    clean = ref["accepted"].copy()
    clean[::2, ::2] = False
    assert np.isfinite(got[clean][:, :3]).all() and np.isfinite(ref["rgb"][clean]).all()
    assert not M.disagreement(got, ref).any()
    shifted = M.synthetic_frames(O, w, h, "drift", seed=7, exotic=False)
    args2 = [shifted["color"], shifted["nd"], args[2], shifted["old_nd"], shifted["cam"], shifted["old_cam"]]
    got2 = O.temporal(*args2, tu, True)
    ref2 = M.temporal_f64(*args2, tu)
    assert np.isnan(got2[ref2["accepted"] & ~ref2["edge"]][:, :3]).all(axis=-1).mean() > 0.5
    assert not M.disagreement(got2, ref2).any()
