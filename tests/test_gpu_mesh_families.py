"""GPU: the mesh families of tests/mesh_families.py through the two voxelisers (include/vxrt_voxelize.h, include/vxrt_solid.h).  Every
comparison is bit for bit against the numpy models' lists, which mesh_families caches: positions, mrgb bytes, order and count, with
no pinned difference.  tests/test_mesh_families_cpu.py checks without a GPU that each family is what it claims, and that the lists
of the combined meshes follow from their families' lists."""
import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import mesh_families as F
import voxelize_model as M
from test_gpu_device_build import assert_same_scene
from test_gpu_edit import make_ctx
from test_gpu_solid import last_error
from test_gpu_solid import raw as raw_solid
from test_gpu_voxelize import CFG, assert_list, guarded, on_device, raw, untouched

pytestmark = pytest.mark.gpu

MODES = [False, True]                # interior_only
MODE_IDS = ["union", "interior"]


@pytest.fixture(scope="module")
def ctx(H):
    with make_ctx(H, CFG) as c:      # no scene is loaded: the voxelisers need none
        yield c


def fresh(mesh):
    """writable copies: the cached meshes are read-only, and torch wants arrays it could write to"""
    return tuple(np.array(a) for a in mesh)


def on_device_mesh(mesh):
    v, t, m = fresh(mesh)
    return on_device(v), on_device(t.view(np.int32)), on_device(m)


def assert_surface(ctx, mesh, want, what):
    """numpy in; tensors in with a cap a few above the count; and the count alone"""
    assert_list(ctx.voxelize_mesh(*fresh(mesh)), want, what)
    dv, dt, dm = on_device_mesh(mesh)
    assert_list(ctx.voxelize_mesh(dv, dt, dm, cap=len(want[0]) + 3), want, f"{what}, tensors and a cap")
    assert raw(ctx, dv, dt, None, None, None, 0) == (0, len(want[0])), f"{what}, count only"


def assert_solid(ctx, mesh, want, interior_only, what):
    assert_list(ctx.voxelize_solid(*fresh(mesh), F.FILL, interior_only=interior_only), want, what)
    dv, dt, dm = on_device_mesh(mesh)
    assert raw_solid(ctx, dv, dt, None, None, int(interior_only), None, None, 0) == (0, len(want[0])), f"{what}, count only"


# ---- the surface -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.SURFACE)
def test_every_surface_family(ctx, name):
    want = F.surface_list(name)
    print(f"surface {name}: {len(want[0])} voxels")
    assert len(want[0]) > 1000
    assert_surface(ctx, F.surface_mesh(name), want, name)


def test_long_segments_past_the_64_cell_mask_from_both_ends(ctx):
    want = F.surface_list("long_segments")
    # what the case is for, on the model's list: columns along x that hold more than 64 set cells, so that the emit pass tests cells
    # again instead of reading their outcome from its mask
    columns = F.long_columns(want[0])
    print(f"long_segments: {columns} columns hold more than 64 set cells")
    assert columns >= F.FLOOR["surface", "long_segments", "columns past the mask"]
    mesh = F.surface_mesh("long_segments")
    assert_list(ctx.voxelize_mesh(*fresh(mesh)), want, "long_segments")
    # (b, a, a): the same voxels, and where segments share one, the colour of the later triangle as before
    assert_surface(ctx, F.reversed_segments(mesh), F.reversed_segments_list(), "long_segments reversed")


def test_all_surface_families_in_one_call(ctx):
    v, t, m = fresh(F.all_surface())
    want = F.all_surface_list()
    print(f"all_surface: {len(t)} triangles, {len(want[0])} voxels, depth {M.depth_of(want[0])}")
    assert len(np.unique(want[1], axis=0)) > 5000        # a colour per triangle, and thousands survive
    assert_surface(ctx, (v, t, m), want, "all_surface")
    assert_list(ctx.voxelize_mesh(v, t.astype(np.int64), m), want, "all_surface, int64 indices")


def test_all_surface_families_the_other_way_round(ctx):
    want = F.all_surface_list(backwards=True)
    assert (want[1] != F.all_surface_list()[1]).any()    # the other family wins the shared voxels
    assert_list(ctx.voxelize_mesh(*fresh(F.all_surface(backwards=True))), want, "all_surface backwards")


# ---- the solid ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interior_only", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("name", F.CLOSED)
def test_every_closed_family(ctx, name, interior_only):
    want = F.closed_list(name, interior_only)
    print(f"closed {name}, {MODE_IDS[interior_only]}: {len(want[0])} voxels")
    if interior_only:
        assert (len(want[0]) == 0) == (name in F.NO_INTERIOR)
    else:
        assert len(want[0]) > 1000
    assert_solid(ctx, F.closed_mesh(name), want, interior_only, name)
    if interior_only and name in F.NO_INTERIOR:          # crossings in every column, pairs of no length: an empty list, status 0
        dv, dt, dm = on_device_mesh(F.closed_mesh(name))
        pos, out = guarded(8)
        assert raw_solid(ctx, dv, dt, dm, F.FILL, 1, pos, out, 8) == (0, 0)
        assert untouched(pos, out)


@pytest.mark.parametrize("interior_only", MODES, ids=MODE_IDS)
def test_all_closed_families_in_one_call(ctx, interior_only):
    want = F.all_closed_list(interior_only)
    print(f"all_closed, {MODE_IDS[interior_only]}: {len(F.all_closed()[1])} triangles, {len(want[0])} voxels")
    assert_solid(ctx, F.all_closed(), want, interior_only, "all_closed")


def test_every_open_mesh(ctx, H):
    refused = 0
    pos, out = guarded(4096)
    for i in range(F.N_OPEN):
        mesh = F.open_mesh(i)
        outcome = F.open_outcome(i)
        dv, dt, dm = on_device_mesh(mesh)
        if outcome[0] == "refused":
            refused += 1
            (x, y), count = outcome[1:]
            for mode in (0, 1):
                for p, o, cap in ((pos, out, len(pos)), (None, None, 0)):
                    rc, n = raw_solid(ctx, dv, dt, dm, F.FILL, mode, p, o, cap)
                    assert rc == H.E_SCENE and n == 0xDEAD, (i, mode, rc, n)
                    text = last_error(ctx)
                    assert "not closed" in text and f"column ({x}, {y}) is crossed {count} times" in text, (i, text)
            assert untouched(pos, out), i
        else:
            for interior_only in MODES:
                assert_solid(ctx, mesh, outcome[2 if interior_only else 1], interior_only, f"open mesh {i}, accepted")
    print(f"open: {refused} of {F.N_OPEN} refused")
    assert refused >= F.FLOOR["open", "refused"] and F.N_OPEN - refused >= F.FLOOR["open", "accepted"]
    # a refusal leaves nothing behind
    for interior_only in MODES:
        assert_solid(ctx, F.closed_mesh("sixteenths"), F.closed_list("sixteenths", interior_only), interior_only, "after the refusals")


# ---- into the scene ----------------------------------------------------------------------------------------------------------------
def test_set_mesh_of_all_surface_equals_the_models_list_through_set_voxels(H):
    want = F.all_surface_list()
    with make_ctx(H, CFG) as dev, make_ctx(H, CFG) as host:
        dev.set_mesh(*fresh(F.all_surface()))
        host.recreate_octree(*fresh(want))
        assert dev.scene_depth == 15
        assert_same_scene(dev, host, "set_mesh of all_surface")
        for a, b in zip(dev.get_voxels(), want):
            assert np.array_equal(a, b)


def test_set_solid_of_far_equals_the_models_list_through_set_voxels(H):
    want = F.closed_list("far", False)
    with make_ctx(H, CFG) as dev, make_ctx(H, CFG) as host:
        dev.set_solid(*fresh(F.closed_mesh("far")), F.FILL)
        host.recreate_octree(*fresh(want))
        assert dev.scene_depth == 15
        assert_same_scene(dev, host, "set_solid of far")
        for a, b in zip(dev.get_voxels(), want):
            assert np.array_equal(a, b)
