"""GPU: the device queries (include/vxrt_query.h) against their rules in Python (tests/query_model.py).

Lookup: every word equal to the voxel model asked at pos + offset in Python integers.  Every case with `leaf` also checks guard words
before and after it, that pos is unchanged, that a second call writes the same bytes, that the count-only and the words-only forms
agree, and that n_present is the number of nonzero words (check_lookup).
Rays: unbounded, the raw 36-byte records equal vxrt_pick's byte for byte; bounded, hit flag, time bits, leaf word and normal bits equal
the oracle's cast_bounded_ray with that bound, with the one pinned difference tests/test_gpu_ray_walk.py allows vxrt_pick (the sign of a
zero time); a hit's voxel is in the model with its leaf word, and the lookup of that voxel returns the same word."""
import ctypes as C

import numpy as np
import pytest
# torch's HIP runtime must be the process's first (host.py: set_voxels_device)
import torch

import query_model as Q
import ray_families as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 0x5A5AA5A5
GUARD_WORDS = 8
HIT_WORDS = 9
N_RAYS = 2000
MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)
_REF = {}


# ---- helpers -----------------------------------------------------------------------------------------------------------------------
def on_device(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def ptr(a):
    if a is None or isinstance(a, C.c_void_p):
        return a
    return C.c_void_p(a.data_ptr() if isinstance(a, torch.Tensor) else a)


def last_error(ctx):
    return (ctx._L.vxrt_last_error() or b"").decode()


class Words:
    """n 32-bit words of device memory between guard words"""
    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD_WORDS,), GUARD, dtype=torch.int32, device=DEV)
        torch.cuda.synchronize()
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * GUARD_WORDS)

    def all(self):
        return self.buf.cpu().numpy().view(np.uint32)

    def guards_hold(self):
        words = self.all()
        return bool((words[:GUARD_WORDS] == GUARD).all()) and bool((words[GUARD_WORDS + self.n:] == GUARD).all())

    def untouched(self):
        return bool((self.all() == GUARD).all())

    def words(self):
        return self.all()[GUARD_WORDS:GUARD_WORDS + self.n].copy()


def raw_lookup(ctx, pos, n, offset, leaf, count=True):
    """The C call over device tensors / raw addresses -> (status, *n_present)."""
    torch.cuda.synchronize()
    got = C.c_size_t(0xDEAD)
    off = None if offset is None else (C.c_int32 * 3)(*[int(v) for v in offset])
    rc = ctx._L.vxrt_lookup_voxels_device(ctx._h, ptr(pos), C.c_size_t(n), off, ptr(leaf), C.byref(got) if count else None)
    return rc, got.value


def raw_pick(ctx, o, d, t, n, out):
    torch.cuda.synchronize()
    return ctx._L.vxrt_pick_device(ctx._h, ptr(o), ptr(d), ptr(t), C.c_size_t(n), ptr(out))


def scene_ref(O, scenes, name):
    """One voxel set's side of the comparison, computed once and shared: model, octree, depth, ray families."""
    if name not in _REF:
        _REF[name] = make_ref(O, name, *R.scene_voxels(name, scenes))
    return _REF[name]


def make_ref(O, family_scene, pos, mrgb):
    octree = O.create_octree(pos, mrgb)
    root_half = R.root_half_of(octree)
    return dict(pos=pos, mrgb=mrgb, octree=octree, depth=int(O.voxel_depth(pos)), model=R.leaf_words(pos, mrgb), root_half=root_half,
                fam=R.scene_families(family_scene, pos, root_half, n=N_RAYS), free={}, bounded={})


def cube_and_shell(depth):
    half = 1 << depth
    g = np.arange(-half - 1, half + 1)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(np.int16)


def check_lookup(ctx, model, depth, pos, offset, what, d_pos=None):
    """One list through every form of the call against the model -> the words."""
    pos = np.ascontiguousarray(pos, np.int16).reshape(-1, 3)
    n = len(pos)
    want, present = Q.lookup(model, depth, pos, offset)
    d_pos = on_device(pos) if d_pos is None else d_pos
    address = d_pos if isinstance(d_pos, C.c_void_p) else (d_pos if n else None)
    leaf, again = Words(n), Words(n)
    assert raw_lookup(ctx, address, n, offset, leaf.ptr) == (0, present), (what, last_error(ctx))
    assert leaf.guards_hold(), f"{what}: guard words around leaf"
    assert np.array_equal(leaf.words().view(np.int32), want), f"{what}: {int((leaf.words().view(np.int32) != want).sum())} of {n} words differ"
    assert present == np.count_nonzero(leaf.words()), what
    assert raw_lookup(ctx, address, n, offset, again.ptr) == (0, present) and again.all().tobytes() == leaf.all().tobytes(), f"{what}: a second call"
    assert raw_lookup(ctx, address, n, offset, None) == (0, present), f"{what}: count only"
    again = Words(n)
    assert raw_lookup(ctx, address, n, offset, again.ptr, count=False) == (0, 0xDEAD) and again.all().tobytes() == leaf.all().tobytes(), f"{what}: words only"
    if isinstance(d_pos, torch.Tensor):
        assert np.array_equal(d_pos.cpu().numpy(), pos), f"{what}: pos was written"
        got, k = ctx.lookup_voxels(d_pos, offset)
        assert got.dtype == torch.int32 and got.device == DEV and tuple(got.shape) == (n,) and k == present, what
        assert np.array_equal(got.cpu().numpy(), want), f"{what}: the wrapper"
        assert ctx.count_present(d_pos, offset) == present, f"{what}: count_present"
    return want


def words_of(mrgb):
    m = np.asarray(mrgb, np.uint32)
    return (np.uint32(0x80000000) | (m[:, 0] & 0x7F) << 24 | m[:, 1] << 16 | m[:, 2] << 8 | m[:, 3]).astype(np.uint32).view(np.int32)


# ---- lookup ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["cube16", "cube32"])
def test_lookup_of_every_cell_and_the_shell(O, H, scenes, scene):
    ref = scene_ref(O, scenes, scene)
    d = ref["depth"]
    cells = cube_and_shell(d)
    with H.Context(32, 32) as ctx:
        ctx.recreate_octree(ref["pos"], ref["mrgb"])
        assert ctx.scene_depth == d
        d_cells = on_device(cells)
        whole = check_lookup(ctx, ref["model"], d, cells, None, scene, d_cells)
        assert np.count_nonzero(whole) == len(ref["pos"])
        for offset in ((0, 0, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1 << d), (Q.INT32_MIN, 0, 0), (0, Q.INT32_MAX, 0), (0, 0, Q.INT32_MIN), (Q.INT32_MAX,) * 3):
            got = check_lookup(ctx, ref["model"], d, cells, offset, f"{scene} + {offset}", d_cells)
            if offset == (0, 0, 1 << d):
                assert 0 < np.count_nonzero(got) < len(ref["pos"])         # half of them outside
            if max(map(abs, offset)) > 1 << 20:
                assert not got.any()                                        # nothing wraps


@pytest.mark.parametrize("scene", ["one_voxel", "empty", "deep15"])
def test_lookup_around_the_voxels_and_at_the_corners_of_int16(O, H, scenes, scene):
    ref = scene_ref(O, scenes, scene)
    d = ref["depth"]
    near = np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
    centres = ref["pos"].astype(np.int64) if len(ref["pos"]) else np.zeros((1, 3), np.int64)
    around = np.clip((centres[:, None, :] + near[None, :, :]).reshape(-1, 3), -32768, 32767)
    corners = np.array([[x, y, z] for x in (-32768, 32767) for y in (-32768, 32767) for z in (-32768, 32767)])
    pos = np.concatenate([around, corners, -corners - 1, [[0, 0, 0], [-1, -1, -1]]]).astype(np.int16)
    with H.Context(32, 32) as ctx:
        ctx.recreate_octree(ref["pos"], ref["mrgb"])
        assert ctx.scene_depth == d and (d == 15) == (scene == "deep15")
        got = check_lookup(ctx, ref["model"], d, pos, None, scene)
        assert np.count_nonzero(got) >= len(ref["pos"]) and (scene != "empty" or not got.any())
        for offset in ((1, 0, 0), (0, -1, 0), (0, 0, 1), (-1, -1, -1), (Q.INT32_MAX, 0, 0), (0, Q.INT32_MIN, 0)):
            check_lookup(ctx, ref["model"], d, pos, offset, f"{scene} + {offset}")
        if scene == "deep15":
            edge = np.array([[32767, 3, -2]], np.int16)
            assert check_lookup(ctx, ref["model"], d, edge, None, "the voxel at 32767")[0] == ref["model"][(32767, 3, -2)]
            assert check_lookup(ctx, ref["model"], d, edge, (1, 0, 0), "32767 + 1 does not wrap")[0] == 0
            assert check_lookup(ctx, ref["model"], d, np.array([[-32768, 3, -2]], np.int16), (-1, 0, 0), "-32768 - 1 does not wrap")[0] == 0
            assert check_lookup(ctx, ref["model"], d, np.array([[32766, 3, -2]], np.int16), (1, 0, 0), "32766 + 1")[0] == ref["model"][(32767, 3, -2)]


@pytest.fixture(scope="module")
def cube32(O, H, scenes):
    ref = scene_ref(O, scenes, "cube32")
    with H.Context(32, 32) as ctx:
        ctx.recreate_octree(ref["pos"], ref["mrgb"])
        yield ctx, ref


def test_lookup_list_lengths_across_a_wave_and_a_block(cube32):
    ctx, ref = cube32
    cells = cube_and_shell(ref["depth"])
    cells = cells[np.random.default_rng(7).permutation(len(cells))]
    for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097):
        got = check_lookup(ctx, ref["model"], ref["depth"], cells[:n], (0, 1, 0), f"{n} entries")
        assert n < 63 or 0 < np.count_nonzero(got) < n
    got = C.c_size_t(0xDEAD)                  # n == 0 touches no pointer and still sets the count
    assert ctx._L.vxrt_lookup_voxels_device(ctx._h, C.c_void_p(8), C.c_size_t(0), None, C.c_void_p(2), C.byref(got)) == 0 and got.value == 0
    assert ctx._L.vxrt_lookup_voxels_device(ctx._h, None, C.c_size_t(0), None, None, None) == 0


def test_lookup_of_repeated_positions(cube32):
    ctx, ref = cube32
    rng = np.random.default_rng(8)
    cells = cube_and_shell(ref["depth"])
    cells = cells[rng.permutation(len(cells))[:3000]]
    pos = np.repeat(cells, rng.integers(1, 5, len(cells)), axis=0)
    pos = pos[rng.permutation(len(pos))]
    got = check_lookup(ctx, ref["model"], ref["depth"], pos, None, "repeats")
    assert np.count_nonzero(got) > len({tuple(p) for p in pos[got != 0].tolist()})     # repeated positions count each time


def test_lookup_of_a_list_at_an_odd_address(cube32):
    ctx, ref = cube32
    cells = cube_and_shell(ref["depth"])[::7]
    n = len(cells)
    for off in (1, 3):
        raw = torch.zeros(6 * n + 8, dtype=torch.uint8, device=DEV)
        raw[off:off + 6 * n] = on_device(cells.view(np.uint8).reshape(-1))
        at = C.c_void_p(raw.data_ptr() + off)
        assert at.value % 2 == 1
        check_lookup(ctx, ref["model"], ref["depth"], cells, (0, 0, -1), f"pos at an address = {off} mod 4", at)
        assert np.array_equal(raw[off:off + 6 * n].cpu().numpy(), cells.view(np.uint8).reshape(-1)) and not raw[:off].any() and not raw[off + 6 * n:].any()


@pytest.mark.parametrize("scene", ["castle", "sponge"])
def test_lookup_of_the_scenes_own_list_is_the_identity(H, scenes, scene):
    with H.Context(32, 32) as ctx:
        if scene == "castle":
            pos, mrgb, _ = scenes.load_scene("castle")
            ctx.recreate_octree(np.ascontiguousarray(pos, np.int16), np.ascontiguousarray(mrgb, np.uint8))
        else:
            ctx.set_menger(3, 0, MENGER_MRGB)                     # built on the device
        p, m = ctx.get_voxels_device()
        n = len(p)
        assert n == ctx.count_voxels() and n > 1000
        leaf, present = ctx.lookup_voxels(p)
        assert present == n and ctx.count_present(p) == n
        assert np.array_equal(leaf.cpu().numpy(), words_of(m.cpu().numpy())) and bool((leaf != 0).all())
        # the same list shifted: what the model of the list says
        model = R.leaf_words(p.cpu().numpy(), m.cpu().numpy())
        check_lookup(ctx, model, ctx.scene_depth, p.cpu().numpy(), (1, 0, 0), f"{scene} + (1, 0, 0)", p)


STATES = ["host", "device", "edited", "compacted", "deeper", "order2", "order3"]


def cube32_in_state(O, H, ctx, ref, state):
    """cube32 brought into `ctx` in one of the ways a tree gets into device memory -> the reference of the voxel set it then holds."""
    pos, mrgb, depth = ref["pos"], ref["mrgb"], ref["depth"]
    if state in ("host", "order2", "order3"):
        ctx.recreate_octree(pos, mrgb)
        assert ctx.stats().node_order == (int(state[-1]) if state.startswith("order") else 0)
        return ref
    if state == "device":
        ctx.set_voxels_device(pos, mrgb)
        return ref
    # a layer cleared and some voxels set (new ones and recoloured ones): holes and 8-entry blocks
    key = "cube32+edits"
    rng = np.random.default_rng(9)
    layer = pos[:, 1] == 3
    free = np.array([c for c in cube_and_shell(depth).tolist() if tuple(c) not in ref["model"] and max(c) < 16 and min(c) >= -16 and c[1] != 3], np.int16)
    added = free[rng.permutation(len(free))[:400]]
    recoloured = pos[~layer][rng.permutation(int((~layer).sum()))[:200]]
    set_pos = np.concatenate([added, recoloured])
    set_mrgb = rng.integers(0, 256, (len(set_pos), 4)).astype(np.uint8)
    set_mrgb[:, 0] &= 0x7F
    ctx.recreate_octree(pos, mrgb)
    ctx.clear_voxels(pos[layer])
    ctx.edit_voxels(set_pos, set_mrgb)
    storage = ctx.scene_storage()
    assert storage["records_used"] > storage["records_live"]
    if state in ("compacted", "deeper"):
        ctx.compact_scene()
        storage = ctx.scene_storage()
        assert storage["records_used"] == storage["records_live"]
    if key not in _REF:
        voxels = {tuple(p): tuple(b) for p, b in zip(pos[~layer].tolist(), mrgb[~layer].tolist())}
        voxels.update({tuple(p): tuple(b) for p, b in zip(set_pos.tolist(), set_mrgb.tolist())})
        new_pos = np.array(sorted(voxels), np.int16)
        new_mrgb = np.array([voxels[k] for k in sorted(voxels)], np.uint8)
        _REF[key] = make_ref(O, "cube32", new_pos, new_mrgb)
        assert _REF[key]["depth"] == depth and len(new_pos) == len(pos) - int(layer.sum()) + len(added)
    assert ctx.count_voxels() == len(_REF[key]["pos"])
    if state == "deeper":
        ctx.set_scene_depth(depth + 1)
        assert ctx.scene_depth == depth + 1
    return _REF[key]


@pytest.mark.parametrize("state", STATES)
def test_lookup_in_every_way_a_tree_gets_into_memory(O, H, scenes, state):
    base = scene_ref(O, scenes, "cube32")
    tuning = [(H.OPT_NODE_ORDER, int(state[-1]))] if state.startswith("order") else []
    with H.Context(32, 32, tuning=tuning) as ctx:
        ref = cube32_in_state(O, H, ctx, base, state)
        depth = ctx.scene_depth
        assert depth == ref["depth"] + (1 if state == "deeper" else 0)
        cells = cube_and_shell(ref["depth"])
        if state == "deeper":       # the old shell is inside the new cube (and empty); the new cube's own shell and corners beside it
            half = 1 << depth
            far = np.random.default_rng(10).integers(-half - 1, half + 1, (4000, 3))
            cells = np.concatenate([cells, far.astype(np.int16)])
        d_cells = on_device(cells)
        got = check_lookup(ctx, ref["model"], depth, cells, None, state, d_cells)
        assert np.count_nonzero(got[:len(cube_and_shell(ref["depth"]))]) == len(ref["pos"])
        check_lookup(ctx, ref["model"], depth, cells, (-1, 0, 1), f"{state} + (-1, 0, 1)", d_cells)


def test_a_detached_piece_is_tested_for_collision(H):
    with H.Context(32, 32) as ctx:
        ctx.set_menger(3, 0, MENGER_MRGB)
        pos, mrgb = ctx.get_voxels()
        assert len(pos) == 8000
        lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
        anchor = (tuple(lo.tolist()), (int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))            # the lowest y layer
        cut = pos[:, 1] == lo[1] + 8
        ctx.clear_voxels_device(on_device(pos[cut]))
        p_pos, _, piece, table = ctx.detached_pieces(*anchor)
        sizes = table["voxels"].cpu().numpy()
        assert sizes.tolist() == [4800]
        largest = int(np.argmax(sizes))
        piece_pos = p_pos.cpu().numpy()[piece.cpu().numpy() == largest]
        assert len(piece_pos) == 4800 and (piece_pos[:, 1] > lo[1] + 8).all()
        d_piece = on_device(piece_pos)
        assert ctx.count_present(d_piece) == 4800                     # still in the scene
        ctx.drop_detached_pieces(*anchor)
        gone = {tuple(p) for p in piece_pos.tolist()}
        model = {k: v for k, v in R.leaf_words(pos[~cut], mrgb[~cut]).items() if k not in gone}
        assert len(model) == ctx.count_voxels() == 8000 - int(cut.sum()) - 4800
        depth = ctx.scene_depth
        assert ctx.count_present(d_piece) == 0 == Q.lookup(model, depth, piece_pos)[1]
        down_one = Q.lookup(model, depth, piece_pos, (0, -1, 0))[1]
        assert ctx.count_present(d_piece, (0, -1, 0)) == down_one == 0           # its lowest layer lies in the cleared one
        down_two = Q.lookup(model, depth, piece_pos, (0, -2, 0))[1]
        assert ctx.count_present(d_piece, (0, -2, 0)) == down_two > 0            # ... and then on what is left standing
        check_lookup(ctx, model, depth, piece_pos, (0, -2, 0), "the piece two down", d_piece)
        check_lookup(ctx, model, depth, piece_pos, (3, -9, 1), "the piece moved into the base", d_piece)


def test_lookup_refusals_write_nothing(cube32, H):
    ctx, ref = cube32
    n = 1025
    pos = cube_and_shell(ref["depth"])[:n].copy()
    d_pos = on_device(pos)
    leaf = Words(n)

    def refused(*args, status=H.E_INVALID, c=ctx, **kw):
        assert raw_lookup(c, *args, **kw) == (status, 0xDEAD), args
        assert last_error(c)
        assert leaf.untouched()

    refused(d_pos, n, None, None, count=False)                                    # both outputs null
    assert "both null" in last_error(ctx)
    refused(C.c_void_p(pos.ctypes.data), n, None, leaf.ptr)                         # pos in host memory, pageable
    assert "pos" in last_error(ctx) and "not device memory" in last_error(ctx)
    refused(torch.as_tensor(pos).pin_memory(), n, None, leaf.ptr)                   # ... and pinned
    refused(None, n, None, leaf.ptr)
    host = np.zeros(n, np.uint32)
    refused(d_pos, n, None, C.c_void_p(host.ctypes.data))                           # leaf in host memory
    assert "leaf" in last_error(ctx) and "not device memory" in last_error(ctx) and not host.any()
    refused(d_pos, n, None, C.c_void_p(leaf.ptr.value + 2))                         # misaligned by 2 bytes
    assert "aligned" in last_error(ctx)
    refused(d_pos, 1 << 32, None, leaf.ptr)                                         # checked before any pointer is looked at
    refused(None, 1 << 32, None, None)
    assert "2^32" in last_error(ctx)
    # leaf one entry short: an allocation of its own, because what the library can see is the allocation (a torch tensor lies in a
    # larger block of torch's allocator); 1024 words are a whole page, so no rounding hides the missing entry
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    assert hip.hipMalloc(C.byref(short), C.c_size_t(4 * (n - 1))) == 0
    refused(d_pos, n, None, short)
    assert "leaf" in last_error(ctx) and "past its allocation" in last_error(ctx)
    assert raw_lookup(ctx, d_pos, n - 1, None, short) == (0, Q.lookup(ref["model"], ref["depth"], pos[:n - 1])[1])     # it holds n - 1
    assert hip.hipFree(short) == 0
    with H.Context(32, 32) as bare:                                                 # no scene
        refused(d_pos, n, None, leaf.ptr, status=H.E_NOSCENE, c=bare)
        with pytest.raises(H.VxrtError) as e:
            bare.lookup_voxels(d_pos)
        assert e.value.status == H.E_NOSCENE
        with pytest.raises(H.VxrtError) as e:
            bare.count_present(d_pos)
        assert e.value.status == H.E_NOSCENE
    # ... and the valid call is accepted afterwards
    check_lookup(ctx, ref["model"], ref["depth"], pos, None, "after the refusals", d_pos)


# ---- rays --------------------------------------------------------------------------------------------------------------------------
def records(p):
    """A pick result (dict of numpy arrays, or of torch tensors) as packed vxrt_pick_hit records."""
    host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in p.items()}
    out = np.zeros(len(host["status"]), hit_dtype())
    for k in out.dtype.names:
        out[k] = host[k]
    return out


def hit_dtype():
    from gpu_voxel_raytracer_amd import host
    assert host.PICK_HIT_DTYPE.itemsize == 4 * HIT_WORDS
    return host.PICK_HIT_DTYPE


def assert_views_of_one_buffer(p, n):
    assert p["status"].dtype == torch.uint32 and p["time"].dtype == torch.float32 and p["normal"].dtype == torch.float32
    assert p["voxel"].dtype == torch.int32 and p["leaf"].dtype == torch.int32 and all(v.device == DEV for v in p.values())
    assert tuple(p["status"].shape) == (n,) and tuple(p["normal"].shape) == (n, 3) and tuple(p["voxel"].shape) == (n, 3) and tuple(p["leaf"].shape) == (n,)
    if n:
        base = p["status"].data_ptr()
        assert [p[k].data_ptr() - base for k in ("time", "normal", "voxel", "leaf")] == [4, 8, 20, 32]
        assert all(p[k].stride(0) == HIT_WORDS for k in p) or n == 1


def oracle_free(O, ref, family):
    if family not in ref["free"]:
        ref["free"][family] = Q.cast(O, ref["octree"], *ref["fam"][family])
    return ref["free"][family]


def oracle_bounded(O, ref, family):
    if family not in ref["bounded"]:
        o, d = ref["fam"][family]
        bounds = Q.dealt_bounds(len(o), ref["root_half"])
        ref["bounded"][family] = (bounds, Q.cast(O, ref["octree"], o, d, bounds))
    return ref["bounded"][family]


def check_rays(O, ctx, ref, what, only=None):
    """pick_device, unbounded and bounded, family by family: against vxrt_pick's bytes, the oracle, the model and the lookup."""
    for family, (o, d) in ref["fam"].items():
        if only is not None and family not in only:
            continue
        n = len(o)
        d_o, d_d = on_device(o), on_device(d)
        free = ctx.pick_device(d_o, d_d)
        assert_views_of_one_buffer(free, n)
        free_rec = records(free)
        host_rec = records(ctx.pick(o, d))
        assert free_rec.tobytes() == host_rec.tobytes(), f"{what}: {family}: unbounded, against vxrt_pick's bytes"
        for name, r in (("unbounded", free_rec), ("vxrt_pick", host_rec)):      # each against the oracle, not through the other
            picked = (r["status"] != 0, r["time"], r["leaf"], r["normal"])
            R.assert_rays_equal(picked, oracle_free(O, ref, family), f"{what}: {family}: {name}", o, d, zero_time_sign=True)
        bounds, want = oracle_bounded(O, ref, family)
        got = ctx.pick_device(d_o, d_d, on_device(bounds))
        rec = records(got)
        assert np.isin(rec["status"], (0, 1, 2)).all()
        R.assert_rays_equal((rec["status"] != 0, rec["time"], rec["leaf"], rec["normal"]), want, f"{what}: {family}: bounded", o, d, zero_time_sign=True)
        assert np.array_equal(rec["status"] == 2, rec["leaf"] == np.int32(-2 ** 31)), f"{what}: {family}: status 2 <=> the cap's leaf word"
        unbounded = bounds == np.float32(Q.UNBOUNDED)
        assert unbounded.sum() >= n // 7 and rec[unbounded].tobytes() == free_rec[unbounded].tobytes(), f"{what}: {family}: a bound of 2^30"
        assert np.array_equal(d_o.cpu().numpy().view(np.uint32), o.view(np.uint32)) and np.array_equal(d_d.cpu().numpy().view(np.uint32), d.view(np.uint32))
        # status 1: the voxel is in the model with that leaf word, and the lookup of the voxel gives the same word
        for r in (free_rec, rec):
            hit = r["status"] == 1
            assert (r["voxel"][~hit] == 0).all()
            if hit.any():
                model_words = np.array([ref["model"].get(tuple(v), 0) for v in r["voxel"][hit].tolist()], np.int32)
                assert np.array_equal(model_words, r["leaf"][hit]), f"{what}: {family}: a picked voxel is not in the model with its leaf word"
                assert np.abs(r["voxel"][hit]).max() <= 32768
                looked, present = ctx.lookup_voxels(on_device(r["voxel"][hit].astype(np.int16)))
                assert present == int(hit.sum()) and np.array_equal(looked.cpu().numpy(), r["leaf"][hit]), f"{what}: {family}: lookup of the picked voxels"


@pytest.mark.parametrize("scene", R.SCENES)
def test_rays_of_every_family(O, H, scenes, scene):
    ref = scene_ref(O, scenes, scene)
    with H.Context(32, 32) as ctx:
        ctx.recreate_octree(ref["pos"], ref["mrgb"])
        assert ctx.scene_depth == ref["depth"]
        before = ctx.stats().rays
        check_rays(O, ctx, ref, scene)
        assert ctx.stats().rays == before


@pytest.mark.parametrize("state", ["edited", "compacted", "order2", "order3"])
def test_rays_in_the_states_of_cube32(O, H, scenes, state):
    from test_gpu_ray_walk import STATE_FAMILIES
    base = scene_ref(O, scenes, "cube32")
    tuning = [(H.OPT_NODE_ORDER, int(state[-1]))] if state.startswith("order") else []
    with H.Context(32, 32, tuning=tuning) as ctx:
        ref = cube32_in_state(O, H, ctx, base, state)
        check_rays(O, ctx, ref, f"cube32 {state}", only=STATE_FAMILIES)


def test_ray_counts_guards_and_repeatability(O, cube32):
    ctx, ref = cube32
    o, d = ref["fam"]["on_planes"]
    bounds = Q.dealt_bounds(len(o), ref["root_half"])
    d_o, d_d, d_t = on_device(o), on_device(d), on_device(bounds)
    whole = records(ctx.pick_device(d_o, d_d, d_t))
    for n in (1, 255, 256, 257):
        out, again = Words(HIT_WORDS * n), Words(HIT_WORDS * n)
        assert raw_pick(ctx, d_o, d_d, d_t, n, out.ptr) == 0, last_error(ctx)
        assert out.guards_hold() and out.words().tobytes() == whole[:n].tobytes(), f"{n} rays"
        assert raw_pick(ctx, d_o, d_d, d_t, n, again.ptr) == 0 and again.all().tobytes() == out.all().tobytes(), f"{n} rays: a second call"
        free = Words(HIT_WORDS * n)
        assert raw_pick(ctx, d_o, d_d, None, n, free.ptr) == 0 and free.guards_hold()
        assert free.words().tobytes() == records(ctx.pick(o[:n], d[:n])).tobytes(), f"{n} rays, unbounded"
    # vxrt_pick through its host entry launches the same kernel in blocks of 256 rays (trace_common.h: kBlock): one ray, one short
    # of a block, a block, one past it and one past two, each against the oracle with the walk test's pinned difference
    want = oracle_free(O, ref, "on_planes")
    for n in (1, 255, 256, 257, 513):
        rec = records(ctx.pick(o[:n], d[:n]))
        assert len(rec) == n
        R.assert_rays_equal((rec["status"] != 0, rec["time"], rec["leaf"], rec["normal"]), tuple(w[:n] for w in want), f"vxrt_pick, {n} rays",
                            o[:n], d[:n], zero_time_sign=True)
    assert ctx._L.vxrt_pick_device(ctx._h, C.c_void_p(4), None, None, C.c_size_t(0), None) == 0        # n == 0 touches no pointer
    none = ctx.pick_device(d_o[:0], d_d[:0], 1.0)
    assert_views_of_one_buffer(none, 0)


def test_a_scalar_max_time_is_the_tensor_of_that_value(O, cube32):
    ctx, ref = cube32
    o, d = ref["fam"]["root_faces"]
    d_o, d_d = on_device(o), on_device(d)
    for value in (4.0, 0.0, 1, -1.0, float("nan"), Q.UNBOUNDED, np.float32(0.25)):
        scalar = records(ctx.pick_device(d_o, d_d, value))
        tensor = records(ctx.pick_device(o, d, torch.full((len(o),), float(value), dtype=torch.float32, device=DEV)))     # numpy rays are uploaded
        assert scalar.tobytes() == tensor.tobytes(), value
        want = Q.cast(O, ref["octree"], o, d, float(value))
        R.assert_rays_equal((scalar["status"] != 0, scalar["time"], scalar["leaf"], scalar["normal"]), want, f"max_time {value}", o, d, zero_time_sign=True)
    # the bounds do bound (the oracle's counts on these rays: 0, 1 247, 1 384 and 1 458; a bound of 4 already reaches every hit)
    hits = [int((records(ctx.pick_device(d_o, d_d, t))["status"] != 0).sum()) for t in (-1.0, 0.25, 1.0, None)]
    assert hits == [int(Q.cast(O, ref["octree"], o, d, t)[0].sum()) for t in (-1.0, 0.25, 1.0, None)]
    assert hits[0] == 0 < hits[1] < hits[2] < hits[3]


def test_pick_refusals_write_nothing(cube32, H):
    ctx, ref = cube32
    n = 1025
    o, d = (np.ascontiguousarray(a[:n]) for a in ref["fam"]["on_planes"])
    t = np.full(n, 4.0, np.float32)
    d_o, d_d, d_t = on_device(o), on_device(d), on_device(t)
    out = Words(HIT_WORDS * n)

    def refused(*args, status=H.E_INVALID, c=ctx):
        assert raw_pick(c, *args) == status, args
        assert last_error(c)
        assert out.untouched()

    host_out = np.zeros(HIT_WORDS * n, np.uint32)
    for args, name in (((C.c_void_p(o.ctypes.data), d_d, d_t, n, out.ptr), "origins"), ((d_o, C.c_void_p(d.ctypes.data), d_t, n, out.ptr), "dirs"),
                       ((d_o, d_d, C.c_void_p(t.ctypes.data), n, out.ptr), "max_time"), ((d_o, d_d, d_t, n, C.c_void_p(host_out.ctypes.data)), "out")):
        refused(*args)                                                               # host memory
        assert name in last_error(ctx) and "not device memory" in last_error(ctx)
    assert not host_out.any()
    refused(torch.as_tensor(o).pin_memory(), d_d, None, n, out.ptr)                 # pinned host memory
    for args in ((None, d_d, d_t, n, out.ptr), (d_o, None, d_t, n, out.ptr), (d_o, d_d, d_t, n, None)):
        refused(*args)
    for args, name in (((C.c_void_p(d_o.data_ptr() + 2), d_d, d_t, n - 1, out.ptr), "origins"), ((d_o, C.c_void_p(d_d.data_ptr() + 2), d_t, n - 1, out.ptr), "dirs"),
                       ((d_o, d_d, C.c_void_p(d_t.data_ptr() + 2), n - 1, out.ptr), "max_time"), ((d_o, d_d, d_t, n - 1, C.c_void_p(out.ptr.value + 2)), "out")):
        refused(*args)                                                               # misaligned by 2 bytes
        assert name in last_error(ctx) and "aligned" in last_error(ctx)
    refused(d_o, d_d, d_t, 1 << 31, out.ptr)                                         # checked before any pointer is looked at
    refused(None, None, None, 1 << 31, None)
    assert "too many rays" in last_error(ctx)
    # out one record short, as an allocation of its own: 1024 records are nine whole pages
    hip = C.CDLL("libamdhip64.so")
    short = C.c_void_p()
    assert 4 * HIT_WORDS * (n - 1) % 4096 == 0 and hip.hipMalloc(C.byref(short), C.c_size_t(4 * HIT_WORDS * (n - 1))) == 0
    refused(d_o, d_d, d_t, n, short)
    assert "out" in last_error(ctx) and "past its allocation" in last_error(ctx)
    assert raw_pick(ctx, d_o, d_d, d_t, n - 1, short) == 0                           # it holds n - 1
    assert hip.hipFree(short) == 0
    with H.Context(32, 32) as bare:                                                  # no scene
        refused(d_o, d_d, d_t, n, out.ptr, status=H.E_NOSCENE, c=bare)
        with pytest.raises(H.VxrtError) as e:
            bare.pick_device(d_o, d_d)
        assert e.value.status == H.E_NOSCENE
    # ... and the valid call is accepted afterwards
    assert raw_pick(ctx, d_o, d_d, d_t, n, out.ptr) == 0 and out.guards_hold()
    assert out.words().tobytes() == records(ctx.pick_device(d_o, d_d, d_t)).tobytes()
