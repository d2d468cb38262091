"""GPU: the device-list entry points that order themselves through Context._ordered() (host.py) are ordered against torch's current
stream on both sides.  Nothing here provokes a fault: a wait that is missing shows as wrong values.

Input side (test_gpu_voxelize.py::test_a_mesh_written_on_a_side_stream_is_read_whole): the arguments are zero-filled tensors of a
side stream that is kept busy before the real data is copied in; the call is made inside that stream's context and has to read the
data, not the zeros (one position, one ray of no length), so its result equals the Python model's of the real data.  rotate_voxels
first reads the list's bounds back with torch on that stream, which waits for the data whatever the library does: its case holds
the bounds to be the data's.

Output side (test_gpu_grid.py::test_export_is_ordered_for_the_next_torch_op): torch's current stream is busy, blocks of the sizes
the call will allocate are filled with a pattern on it and freed, so that the caching allocator hands the call's output tensors
memory whose fill is still pending; the call has to wait for that fill before it writes, and the torch reduction that follows at
once, with no synchronize, has to wait for the call.  Three rounds; the digest of every output equals the model's.

What notices what (MI355X, each wait of Context._ordered() turned into a no-op in the test process alone).  Without the wait in
front of the call, every input case fails but rotate_voxels', and the output cases of get_voxels_device, lookup_voxels and
label_components fail; those of detached_voxels, detached_pieces and transform_voxels do not, because these first count, the host
waits for the count, and by then torch's stream has filled the blocks.  Without the wait behind the call none fails: every one of
these entry points hands a count back to the host or is followed by a read-back that waits, so its work is done when the result is
looked at; the cases hold the results right all the same."""
import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import components_model as K
import edit_model as M
import pieces_model as P
import query_model as Q
import transform_model as T

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SLEEP_IN, SLEEP_OUT = 50_000_000, 20_000_000       # the cycles the two tests named above keep their streams busy for
N_RAYS = 2000
ROUNDS = 3


def on_device(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return None if t is None else t.cpu().numpy()


def written_late(*arrays):
    """-> (side stream, tensors): zero-filled tensors of the side stream, which is busy first and copies the arrays in afterwards.
    The caller makes its call inside `torch.cuda.stream(side)`."""
    sources = [on_device(a) for a in arrays]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        tensors = [torch.zeros_like(s) for s in sources]
        torch.cuda._sleep(SLEEP_IN)                 # the producer is still busy when the call is made
        for t, s in zip(tensors, sources):
            t.copy_(s)
    return side, tensors


def sparse_cells(seed, n=3000, side=24):
    """n entries at random cells of [0, side)^3 (so some positions repeat) with random bytes; entry 0 is not at the origin"""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, side, (n, 3)).astype(np.int16)
    pos[0] = (side - 1, 1, 2)
    return pos, rng.integers(0, 256, (n, 4)).astype(np.uint8)


@pytest.fixture(scope="module")
def sponge(H):
    """the level-3 sponge with a colour per voxel -> (context, model {pos: word}, depth)"""
    pos, _ = H.menger_voxels(3)
    mrgb = np.random.default_rng(21).integers(0, 256, (len(pos), 4)).astype(np.uint8)
    with H.Context(96, 64) as ctx:
        ctx.recreate_octree(pos, mrgb)
        yield ctx, M.from_list(pos, mrgb), ctx.scene_depth


@pytest.fixture(scope="module")
def cut_sponge(H):
    """the same sponge without its layer y = 8, anchored at its lowest layer: what lies above the cut is one detached piece
    -> (context, voxels {pos: (m, r, g, b)}, depth, anchor)"""
    pos, _ = H.menger_voxels(3)
    mrgb = np.random.default_rng(22).integers(0, 256, (len(pos), 4)).astype(np.uint8)
    lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
    keep = pos[:, 1] != lo[1] + 8
    pos, mrgb = pos[keep], mrgb[keep]
    anchor = (tuple(lo.tolist()), (int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))
    voxels = {tuple(p): (c[0] & 0x7F, c[1], c[2], c[3]) for p, c in zip(pos.tolist(), mrgb.tolist())}
    with H.Context(32, 32) as ctx:
        ctx.recreate_octree(pos, mrgb)
        yield ctx, voxels, ctx.scene_depth, anchor


@pytest.fixture(scope="module")
def bare(H):
    with H.Context(32, 32) as ctx:
        yield ctx


def query_positions(depth, seed, n=4000):
    """positions in and one cell around the root cube; entry 0 is outside it, where the origin is a voxel of the sponge"""
    half = 1 << depth
    pos = np.random.default_rng(seed).integers(-half - 1, half + 1, (n, 3)).astype(np.int16)
    pos[0] = (half, 0, 0)
    return pos


# ---- input side --------------------------------------------------------------------------------------------------------------------
def test_label_components_reads_a_list_written_on_a_side_stream(bare):
    pos, _ = sparse_cells(31)
    connectivity = 6
    want, count = K.label(pos, connectivity)
    assert 1 < count < len(pos)                                      # the zeros are one component
    side, (d_pos,) = written_late(pos)
    with torch.cuda.stream(side):
        label, n = bare.label_components(d_pos, connectivity)
    assert n == count and np.array_equal(host(label), want)


def test_component_table_reads_a_list_written_on_a_side_stream(bare):
    pos, _ = sparse_cells(32)
    want_label, want_id, want_table = P.component_table(pos, 18)
    assert 1 < len(want_table) < len(pos)
    side, (d_pos,) = written_late(pos)
    with torch.cuda.stream(side):
        label, ids, table = bare.component_table(d_pos, 18)
    assert np.array_equal(host(label), want_label) and np.array_equal(host(ids), want_id)
    for f in P.FIELDS:
        assert np.array_equal(host(table[f]), want_table[f]), f


def test_lookup_voxels_reads_positions_written_on_a_side_stream(sponge):
    ctx, model, depth = sponge
    pos = query_positions(depth, 33)
    want, present = Q.lookup(model, depth, pos, (1, -2, 0))
    assert 0 < present < len(pos) and Q.lookup(model, depth, np.zeros_like(pos), (1, -2, 0))[1] in (0, len(pos))
    side, (d_pos,) = written_late(pos)
    with torch.cuda.stream(side):
        leaf, n = ctx.lookup_voxels(d_pos, (1, -2, 0))
    assert n == present and np.array_equal(host(leaf), want)


def test_count_present_reads_positions_written_on_a_side_stream(sponge):
    ctx, model, depth = sponge
    pos = query_positions(depth, 34)
    present = Q.lookup(model, depth, pos)[1]
    assert 0 < present < len(pos) and Q.lookup(model, depth, np.zeros_like(pos))[1] == len(pos)
    side, (d_pos,) = written_late(pos)
    with torch.cuda.stream(side):
        n = ctx.count_present(d_pos)
    assert n == present


def test_pick_device_reads_rays_and_bounds_written_on_a_side_stream(H, scenes, sponge):
    from gpu_voxel_raytracer_amd.host import PICK_HIT_DTYPE
    ctx, model, depth = sponge
    ctx.camera = H.Camera(*scenes.close_camera((27, 27, 27)))
    rng = np.random.default_rng(35)
    o, d = ctx.pixel_rays(rng.uniform(0, ctx.width, N_RAYS), rng.uniform(0, ctx.height, N_RAYS))
    bound = np.full(N_RAYS, Q.UNBOUNDED, np.float32)                 # unbounded: the bytes of pick (a bound of zero ends every ray)
    want = ctx.pick(o, d)
    assert int((want["status"] == H.PICK_HIT).sum()) > N_RAYS // 4
    side, (d_o, d_d, d_t) = written_late(o, d, bound)
    with torch.cuda.stream(side):
        got = ctx.pick_device(d_o, d_d, d_t)
    for name in PICK_HIT_DTYPE.names:
        assert np.ascontiguousarray(host(got[name])).tobytes() == np.ascontiguousarray(want[name]).tobytes(), name


def motion(pos):
    lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
    centre = tuple(((lo + hi + 1) / 2).tolist())
    return lo, hi, T.GENERAL_ROTATIONS[0], centre, (3, -2, 1.5)


def test_transform_voxels_reads_a_list_written_on_a_side_stream(H, bare):
    pos, mrgb = sparse_cells(36)
    lo, hi, r, centre, shift = motion(pos)
    pull, box = H.rigid_pull(r, centre, shift), H.rigid_box(lo, hi, r, centre, shift)
    want = T.transform_np(pos, mrgb, [list(row) for row in pull.m], list(pull.t), *box)
    assert len(want[0]) > 1000
    side, (d_pos, d_mrgb) = written_late(pos, mrgb)
    with torch.cuda.stream(side):
        got = bare.transform_voxels(d_pos, d_mrgb, pull, *box)
    assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1])


def test_rotate_voxels_reads_a_list_written_on_a_side_stream(H, bare):
    """the wrapper first takes the list's bounds with torch, on the same stream: of the data, not of the zeros"""
    pos, mrgb = sparse_cells(37)
    lo, hi, r, centre, shift = motion(pos)
    pull, box = H.rigid_pull(r, centre, shift), H.rigid_box(lo, hi, r, centre, shift)
    want = T.transform_np(pos, mrgb, [list(row) for row in pull.m], list(pull.t), *box)
    assert len(want[0]) > 1000
    side, (d_pos, d_mrgb) = written_late(pos, mrgb)
    with torch.cuda.stream(side):
        got = bare.rotate_voxels(d_pos, d_mrgb, r, centre, shift)
    assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1])


# ---- output side -------------------------------------------------------------------------------------------------------------------
def digest_np(a):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1).astype(np.int64)
    return int((b * (np.arange(len(b), dtype=np.int64) % 251 + 1)).sum())


def consumed_at_once(call, want):
    """ROUNDS times: torch's stream busy, pattern-filled blocks of the outputs' sizes freed on it, the call, and a torch reduction
    of every output right behind it; want: the model's arrays, one per output tensor"""
    sizes = [np.ascontiguousarray(w).nbytes for w in want]
    weights = torch.arange(max(sizes), dtype=torch.int64, device=DEV) % 251 + 1
    digests = [digest_np(w) for w in want]
    torch.cuda.synchronize()
    for k in range(ROUNDS):
        torch.cuda._sleep(SLEEP_OUT)                                # torch's stream is busy when the call is made
        for n in sizes:
            junk = torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV)
            del junk                                                # the allocator may hand this block to the call; its fill is pending
        got = call()
        sums = [(t.contiguous().view(torch.uint8).reshape(-1).to(torch.int64) * weights[:t.numel() * t.element_size()]).sum() for t in got]
        assert [tuple(t.shape) for t in got] == [w.shape for w in want], f"round {k}"
        assert [int(s.item()) for s in sums] == digests, f"round {k}: the outputs' digests differ from the model's"
        for t, w in zip(got, want):
            assert host(t).tobytes() == np.ascontiguousarray(w).tobytes(), f"round {k}"


def test_get_voxels_device_is_ordered_for_the_next_torch_op(sponge):
    import extract_model as X
    ctx, model, depth = sponge
    want = X.ordered_list(model, depth)
    assert len(want[0]) == 8000
    consumed_at_once(lambda: ctx.get_voxels_device(), want)


def test_detached_voxels_is_ordered_for_the_next_torch_op(cut_sponge):
    ctx, voxels, depth, anchor = cut_sponge
    want = K.detached(voxels, *anchor, 6)
    assert len(want[0]) == 4800
    consumed_at_once(lambda: ctx.detached_voxels(*anchor), want)


def test_detached_pieces_is_ordered_for_the_next_torch_op(cut_sponge):
    ctx, voxels, depth, anchor = cut_sponge
    pos, mrgb, piece, table = P.detached_pieces(voxels, *anchor, 6)
    assert len(pos) == 4800 and table["voxels"].tolist() == [4800]

    def call():
        got = ctx.detached_pieces(*anchor)
        return list(got[:3]) + [got[3][f] for f in P.FIELDS]
    consumed_at_once(call, [pos, mrgb, piece] + [np.ascontiguousarray(table[f]) for f in P.FIELDS])


def test_lookup_voxels_is_ordered_for_the_next_torch_op(sponge):
    ctx, model, depth = sponge
    pos = query_positions(depth, 38)
    want, present = Q.lookup(model, depth, pos)
    assert 0 < present < len(pos)
    d_pos = on_device(pos)
    consumed_at_once(lambda: [ctx.lookup_voxels(d_pos)[0]], [want])


def test_label_components_is_ordered_for_the_next_torch_op(bare):
    pos, _ = sparse_cells(39)
    want, count = K.label(pos, 6)
    d_pos = on_device(pos)
    consumed_at_once(lambda: [bare.label_components(d_pos)[0]], [want])


def test_transform_voxels_is_ordered_for_the_next_torch_op(H, bare):
    pos, mrgb = sparse_cells(40)
    lo, hi, r, centre, shift = motion(pos)
    pull, box = H.rigid_pull(r, centre, shift), H.rigid_box(lo, hi, r, centre, shift)
    want = T.transform_np(pos, mrgb, [list(row) for row in pull.m], list(pull.t), *box)
    d_pos, d_mrgb = on_device(pos), on_device(mrgb)
    consumed_at_once(lambda: bare.transform_voxels(d_pos, d_mrgb, pull, *box), want)
