"""Random sequences over every call that changes a loaded scene in place, and their effect on the edit model's dict
({(x, y, z): leaf word}, tests/edit_model.py).  Pure Python and numpy: the GPU test (test_gpu_mutator_sequences.py) replays a
sequence on a context, the CPU test (test_mutator_sequences_cpu.py) checks the generator itself.

sequence(seed, model, depth) yields Step(kind, args, apply_to_model).  The fourteen kinds are KINDS; args names the call's arguments
(args["call"] tells which entry point of the kind, see the GPU test's `run`), and
  args["twin"]   the same step through edit_voxels / clear_voxels / set_scene_depth / fit_scene_depth / compact_scene only, as a list
                 of ("set", pos, mrgb) / ("clear", pos) / ("depth", d) / ("fit",) / ("compact",),
  args["depth"]  the scene's depth after the step,
  args["grows"]  whether the step may leave the root cube it starts in.
apply_to_model(model) applies the step to a dict in place (through edit_model.apply) and returns it.  What a step does to the dict
comes from the models the suite has: edit_model.apply for the lists, grid_edit_model.edit_lists for the grids, voxelize_model.voxelize
and solid_model.solid for the meshes (computed once per shape at the origin and moved by whole voxels, which the rules commute with:
the CPU test checks that against the models of the moved meshes); components_model.detached and pieces_model.detached_pieces for
the two drops; the depth from host.cube_depth / host.scene_depth_for.

Drops.  A drop_detached or drop_detached_pieces step draws a connectivity and an anchor: an axis, the median of the present voxels'
coordinate on it as the cut, and which side of the cut is anchored; the anchor box is that half-space clipped to [-32768, 32768)^3,
so about half of the scene is anchored and what does not hang on that half is removed.  drop_detached_pieces also draws min_voxels /
max_voxels from the sizes of the model's detached pieces (with two distinct sizes or more the range selects some pieces and leaves
one behind) and a cap: None, the exact count or a few more.  A draw that would leave fewer than KEEP voxels (of a scene that holds as many) is drawn again, eight
times at the most; then the half that holds the most voxels is anchored, over every axis and side (and the whole range where even
that leaves fewer, so that nothing is removed).  args holds the call's arguments and the values it returns: pos and mrgb in path
order, for the pieces also piece and table (pieces_model.PIECE records).  A drop is a clear of its list: the twin is ("clear", pos),
and the depth and the far bookkeeping stay.

Order.  The kinds of one seed follow an Eulerian circuit of the complete directed graph on the fourteen kinds with its self-loops: 196
edges, so 197 steps, the first kind once more at the end, and every ordered pair (A directly followed by B) occurs exactly once
among them.  The circuit starts at set_host, so that the smallest start scene holds more than its one voxel before anything clears.

Chunk boundary.  After the first compact, before a set_host or set_device step of the circuit the generator chooses, it inserts a set
of 1023, 1024, 1025 or 2049 voxels (each count once per seed; args["boundary"] is the count) and the clear of the same positions,
through the host lists before a set_host and through the device lists before a set_device.  Every position has even coordinates and
a leaf parent (pos >> 1) of its own that the model does not hold, so every leaf-level segment of edit_kernel allocates and its
1024-segment chunks end one short of, at and one past a full chunk, and two chunks and one segment.  The inserted pair stands between X
and a set step and begins with a set step of the same kind, so the pair (X, set) still occurs.  They need a cube of 2^15 leaf
parents: a slot whose depth is below 5 is passed over, and counts left at the end of the circuit are appended after a depth step.
"""
import collections
import functools

import numpy as np

import components_model as K
import edit_model as M
import extract_model as X
import grid_edit_model as GE
import pieces_model as P
import solid_model as S
import voxelize_model as V
from gpu_voxel_raytracer_amd import host as H
from gpu_voxel_raytracer_amd import scenes

KINDS = ("set_host", "clear_host", "set_device", "clear_device", "grid_replace", "grid_mask", "depth", "far_set", "fit", "compact",
         "mesh", "carve", "drop_detached", "drop_detached_pieces")
BOUNDARY_COUNTS = (1023, 1024, 1025, 2049)
BOUNDARY_DEPTH = 5
KEEP = 4            # voxels a clearing step always leaves, so that a later carve finds one to clear and one to leave
ANCHOR_DRAWS = 8    # anchors a drop step draws before it takes the half that holds the most voxels

Step = collections.namedtuple("Step", "kind args apply_to_model")


def circuit(rng):
    """-> the 197 kinds of an Eulerian circuit over KINDS x KINDS from set_host (Hierholzer, the edges of every kind shuffled)."""
    out = {k: [KINDS[i] for i in rng.permutation(len(KINDS))] for k in KINDS}
    stack, order = [KINDS[0]], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            order.append(stack.pop())
    order.reverse()
    assert len(order) == len(KINDS) ** 2 + 1 and order[0] == order[-1] == KINDS[0]
    return order


@functools.lru_cache(maxsize=None)
def shape(name, radius):
    """An icosphere of that radius around (0.5, 0.5, 0.5) or the cube [0, radius]^3, on the snapping grid -> (verts, tris, surface positions, interior positions): the models' lists"""
    v, t = V.icosphere(int(name[-1]), radius=float(radius)) if name.startswith("icosphere") else V.cube(0.0, float(radius))
    v = (np.rint(v.astype(np.float64) * 16) / 16).astype(np.float32)
    surface = V.voxelize(v, t, (0, 0, 0, 0))[0].astype(np.int64)
    inner = S.solid(v, t, None, (0, 0, 0, 0), interior_only=True)[0].astype(np.int64)
    return v, t, surface, inner


def union_list(surface, inner, mrgb, fill):
    """solid_model.solid's union over the two lists of a shape: the surface's voxels with mrgb, the interior cells it lacks with fill"""
    have = set(map(tuple, surface.tolist()))
    extra = np.array([c for c in map(tuple, inner.tolist()) if c not in have], np.int64).reshape(-1, 3)
    fill = np.array(fill, np.uint8) & np.array([0x7F, 0xFF, 0xFF, 0xFF], np.uint8)
    surf = np.broadcast_to(np.array(mrgb, np.uint8) & np.array([0x7F, 0xFF, 0xFF, 0xFF], np.uint8), (len(surface), 4))
    return np.concatenate([surface, extra]), np.concatenate([surf, np.broadcast_to(fill, (len(extra), 4))])


def applier(delta):
    def apply_to_model(model):
        for d in delta:
            M.apply(model, d[1], d[2] if d[0] == "set" else None)
        return model
    return apply_to_model


def natural_depth(model):
    return H.scene_depth_for(np.array(list(model), np.int64).reshape(-1, 3))


def holding_depth(model):
    """the least depth whose root cube holds every voxel of the model (0 for none)"""
    if not model:
        return 0
    p = np.array(list(model), np.int64)
    return H.cube_depth(p.min(axis=0), p.max(axis=0))


# the start scenes of the GPU test with the seed of each (one seed per scene): the device-built level-3 sponge, castle.vox and the one
# voxel (0, 0, 0), whose depth is 0.  The sponge's seed is the lowest whose first case holds a far_set that has to grow, which the GPU
# test first makes without grow; that it is also the one-voxel scene's seed gives the two the same circuit and nothing else
CASES = (("menger_device", 3), ("castle", 2), ("one_voxel", 3))
MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)
PARTS = 5           # the GPU test runs a sequence as this many consecutive cases (test_gpu_mutator_sequences.py says why)


def part_range(n, part):
    """-> (first, last): the steps case `part` of a sequence of n steps makes on the device.  Case k covers [n k / PARTS,
    n (k + 1) / PARTS) and starts one step before that, so that the ordered pair that straddles two cases is made directly too."""
    return max(n * part // PARTS - 1, 0), n * (part + 1) // PARTS


def refusal_step(steps, depth, first, last):
    """-> the index of the first far_set in [first, last) that has to grow (the GPU test first makes it without grow), or None;
    depth: the scene's depth before step 0"""
    for i, s in enumerate(steps[:last]):
        if i >= first and s.kind == "far_set" and s.args["depth"] > depth:
            return i
        depth = s.args["depth"]
    return None


def start_model(host, scenes, name):
    """host, scenes: the package's host and scenes modules (the test fixtures H and scenes).
    -> (voxel list pos, mrgb; the model dict; the depth the scene is loaded with)"""
    if name == "menger_device":
        pos, mrgb = host.menger_voxels(3, MENGER_MRGB)
    elif name == "one_voxel":
        pos, mrgb = np.zeros((1, 3), np.int16), np.array([[1, 200, 100, 50]], np.uint8)
    else:
        pos, mrgb, _ = scenes.load_scene(name)
    return pos, mrgb, M.from_list(pos, mrgb), host.scene_depth_for(pos)


STEPS = len(KINDS) ** 2 + 1 + 2 * len(BOUNDARY_COUNTS)     # of every sequence, or one more: the depth step before boundary batches left over
_SEQUENCES = {}


def steps_of(name, seed, upto=None):
    """-> (start model, start depth, the steps of the scene's sequence generated so far: the first `upto` at the least, all of them
    for None).  A sequence is generated once per process and only as far as it is asked for, so that each case of the GPU test pays
    for its own steps; the list grows in place and is not the caller's to change."""
    if (name, seed) not in _SEQUENCES:
        _, _, model, depth = start_model(H, scenes, name)
        _SEQUENCES[name, seed] = (model, depth, sequence(seed, model, depth), [])
    model, depth, rest, steps = _SEQUENCES[name, seed]
    while upto is None or len(steps) < upto:
        step = next(rest, None)
        if step is None:
            break
        steps.append(step)
    return model, depth, steps


def part_of(name, seed, part):
    """-> (start model, start depth, steps, first, last): case `part` of the GPU test makes steps[first:last] on the device.  The
    parts divide STEPS (part_range); the last one runs to the sequence's end, and only it generates the whole sequence."""
    first, last = part_range(STEPS, part)
    model, depth, steps = steps_of(name, seed, None if part == PARTS - 1 else last)
    return model, depth, steps, first, (len(steps) if part == PARTS - 1 else last)


def core_depth(start_model):
    """the cube a sequence counts as the scene's own: the start scene's, and depth 4 at the least; voxels set outside it are far"""
    return max(holding_depth(start_model), 4)


def far_voxels(model, core):
    """-> int16 [n, 3]: the model's voxels outside the core cube, which the GPU test clears before its last fit (all but the first of
    them where the core cube holds nothing, so that the scene does not end empty)"""
    half = 1 << core
    out = sorted(p for p in model if min(p) < -half or max(p) >= half)
    return np.array(out[1:] if len(out) == len(model) else out, np.int64).reshape(-1, 3).astype(np.int16)


def sequence(seed, model, depth):
    rng = np.random.default_rng(seed)
    m, far = dict(model), set()               # far: the voxels set outside the core cube, which a fit may clear first
    state = {"depth": int(depth), "core": core_depth(model)}
    pos16 = lambda p: np.asarray(p, np.int64).reshape(-1, 3).astype(np.int16)   # noqa: E731
    colours = lambda n: rng.integers(0, 256, size=(n, 4)).astype(np.uint8)   # noqa: E731

    def emit(kind, args, delta, twin, depth_after=None, grows=False):
        delta = [d for d in delta if len(d[1])]
        args = dict(args, twin=[t for t in twin if t[0] not in ("set", "clear") or len(t[1])],
                    depth=state["depth"] if depth_after is None else int(depth_after), grows=grows)
        apply = applier(delta)
        for d in delta:
            if d[0] == "set":
                p = d[1].astype(np.int64)
                half = 1 << state["core"]
                far.update(map(tuple, p[np.any((p < -half) | (p >= half), axis=1)].tolist()))
        apply(m)
        state["depth"] = args["depth"]
        return Step(kind, args, apply)

    def present(n):
        keys = sorted(m)
        if not keys:
            return np.zeros((0, 3), np.int64)
        return np.array([keys[i] for i in rng.choice(len(keys), size=min(n, len(keys)), replace=False)], np.int64).reshape(-1, 3)

    def set_list():
        """in-cube sets: anywhere, near the scene, a new branch in an empty octant of the root, recolours of present voxels"""
        lim = 1 << state["depth"]
        parts = [rng.integers(-lim, lim, size=(6, 3))]
        if m:
            keys = np.array(list(m), np.int64)
            lo, hi = np.maximum(keys.min(axis=0) - 2, -lim), np.minimum(keys.max(axis=0) + 3, lim)
            parts.append(rng.integers(lo, hi, size=(10, 3)))
            occupied = {tuple(o) for o in np.unique((keys >= 0).astype(np.int64), axis=0).tolist()}
            empty = [o for o in np.ndindex(2, 2, 2) if o not in occupied]
            if empty:
                corner = np.where(np.array(empty[int(rng.integers(len(empty)))]) == 1, 0, -lim)
                parts.append(corner + rng.integers(0, lim, size=(6, 3)))
            parts.append(present(12))
        return np.concatenate(parts)

    def clear_list():
        """present single voxels, one aligned 4^3 or 8^3 cell whole, absent positions; never the whole scene"""
        lim = 1 << state["depth"]
        parts = [present(8), rng.integers(-lim, lim, size=(5, 3))]
        if m:
            side = int(rng.choice([4, 8]))
            cell = (present(1)[0] // side) * side
            box = cell + np.array(list(np.ndindex(side, side, side)), np.int64)
            parts.append(box[np.all((box >= -lim) & (box < lim), axis=1)])
        pos = np.concatenate(parts)
        keep = {tuple(p) for p in present(KEEP).tolist()}         # these stay whatever the cell holds
        return np.array([p for p in pos.tolist() if tuple(p) not in keep], np.int64).reshape(-1, 3)

    def with_duplicates(pos):
        return np.concatenate([pos, pos[:4], pos[-3:]]) if len(pos) else pos

    def grid(mode):
        """a box of random size at a random origin near the scene, about half occupied (WORD32: junk below bit 31 is empty)"""
        lim = 1 << state["depth"]
        for _ in range(8):
            dims = tuple(int(d) for d in rng.integers(1, 21, size=3))
            near = present(1)[0] if m and rng.random() < 0.8 else rng.integers(-lim, lim, size=3)
            origin = tuple(int(v) for v in near - rng.integers(0, np.array(dims) + 1))
            words = (rng.integers(0, 1 << 31, dims) | (1 << 31)).astype(np.uint32).view(np.int32)
            junk = rng.integers(0, 1 << 31, dims).astype(np.int32)
            occupied = rng.random(dims) < 0.5
            if mode != "clear":
                occupied &= GE.in_cube(origin, dims, state["depth"])
            for p in (present(KEEP) - np.array(origin)).tolist():        # these stay: set by a replace, not cleared by a clear
                if all(0 <= c < dm for c, dm in zip(p, dims)):
                    occupied[tuple(p)] = mode == "replace"
            cells = np.where(occupied, words, junk).astype(np.int32)
            cpos, spos, swords, after = GE.edit_lists(m, cells, origin, mode, state["depth"])
            if len(after) >= min(len(m), 2):
                break
        else:
            raise AssertionError("no grid leaves two voxels")
        mrgb = GE.mrgb_of_words(swords)
        return ({"call": "grid", "cells": cells, "origin": origin, "mode": mode},
                [("clear", cpos), ("set", spos, mrgb)], [("clear", cpos), ("set", spos, mrgb)])

    def far_positions(n):
        """voxels past the current cube (one level up); at depth 15 the far corner regions of the cube itself"""
        d = state["depth"]
        lim = 1 << d
        if d == 15:
            p = rng.integers(-lim, lim, size=(n, 3))
            p[:, 0] = np.where(rng.random(n) < 0.5, rng.integers(-lim, -lim // 2, n), rng.integers(lim // 2, lim, n))
            return p
        p = rng.integers(-2 * lim, 2 * lim, size=(n, 3))
        ax = rng.integers(0, 3, n)
        p[np.arange(n), ax] = np.where(rng.random(n) < 0.5, rng.integers(-2 * lim, -lim, n), rng.integers(lim, 2 * lim, n))
        return p

    def place(cells, overlap):
        """a whole-voxel shift that puts the cells inside the root cube where they fit (near a present voxel for `overlap`) -> the
        shift, and whether the cells still leave the cube"""
        lim = 1 << state["depth"]
        lo, hi = cells.min(axis=0), cells.max(axis=0)
        centre = present(1)[0] if m and overlap else rng.integers(-lim, lim, size=3)
        fits = bool(np.all(hi - lo < 2 * lim))
        shift = np.clip(centre, -lim - lo, lim - 1 - hi) if fits else centre
        return shift.astype(np.int64), not fits

    def leaf_parents():
        return {(x >> 1, y >> 1, z >> 1) for x, y, z in m}

    def room(count):
        """the cube holds 2^15 leaf parents or more, and twice the batch of them are empty"""
        d = state["depth"]
        return d >= BOUNDARY_DEPTH and (d > 6 or (1 << (3 * d)) - len(leaf_parents()) >= 2 * count)

    def boundary_pair(count, device):
        d = state["depth"]
        half = 1 << (d - 1)                                          # leaf parents per axis: 2^d, cells [-half, half)
        seen, free = leaf_parents(), []
        for _ in range(64):
            for c in map(tuple, rng.integers(-half, half, size=(4 * count, 3)).tolist()):
                if c not in seen and len(free) < count:
                    seen.add(c)
                    free.append(c)
            if len(free) == count:
                break
        assert len(free) == count, "too few empty leaf parents"
        free = np.array(free, np.int64)
        pos, mrgb = pos16(2 * free), colours(count)
        kind = ("set_device", "clear_device") if device else ("set_host", "clear_host")
        call = "device" if device else "host"
        yield emit(kind[0], {"call": call, "pos": pos, "mrgb": mrgb, "boundary": count}, [("set", pos, mrgb)], [("set", pos, mrgb)])
        yield emit(kind[1], {"call": call, "pos": pos, "boundary": count}, [("clear", pos)], [("clear", pos)])

    def half_space(axis, cut, upper):
        lo, hi = [-32768] * 3, [32768] * 3
        if upper:
            lo[axis] = cut
        else:
            hi[axis] = cut
        return tuple(lo), tuple(hi)

    def drop(pieces):
        """the arguments of a drop and what it returns, from the two models (the docstring's "Drops")"""
        keys = np.array(sorted(m), np.int64).reshape(-1, 3)
        medians = [int(np.sort(keys[:, ax])[len(keys) // 2]) for ax in range(3)]
        pos, mrgb = M.to_list(m)
        voxels = {tuple(p): tuple(c) for p, c in zip(pos.tolist(), mrgb.tolist())}
        conn = int(rng.choice(K.CONNECTIVITIES))

        def chosen(anchor):
            """-> what the call returns with this anchor, and its remaining arguments"""
            if not pieces:
                return K.detached(voxels, *anchor, conn), {}
            got = P.detached_pieces(voxels, *anchor, conn)
            sizes = sorted(set(got[3]["voxels"].tolist()))
            least, most = 0, None
            if len(sizes) >= 2:          # sizes[i] .. sizes[j], never the whole range: a detached piece stays
                i, j = sorted(int(v) for v in rng.integers(0, len(sizes), 2))
                if (i, j) == (0, len(sizes) - 1):
                    i, j = ((1, j) if rng.random() < 0.5 else (0, j - 1))
                least = sizes[i] if i > 0 or rng.random() < 0.5 else 0
                most = sizes[j] if j < len(sizes) - 1 or rng.random() < 0.5 else None
                got = P.detached_pieces(voxels, *anchor, conn, least, P.EVERY if most is None else most)
            cap = (None, len(got[0]), len(got[0]) + int(rng.integers(1, 6)))[int(rng.integers(3))]
            return got, {"min_voxels": least, "max_voxels": most, "cap": cap}

        floor = min(KEEP, len(m))
        for _ in range(ANCHOR_DRAWS):
            axis, upper = int(rng.integers(3)), bool(rng.integers(2))
            anchor = half_space(axis, medians[axis], upper)
            got, more = chosen(anchor)
            if len(m) - len(got[0]) >= floor:
                break
        else:
            held = lambda a: int(X.in_box(keys, a).sum())   # noqa: E731
            anchor = max((half_space(ax, medians[ax], up) for ax in range(3) for up in (False, True)), key=held)
            got, more = chosen(anchor)
            if len(m) - len(got[0]) < floor:
                anchor = ((-32768,) * 3, (32768,) * 3)
                got, more = chosen(anchor)
        args = dict(more, call="drop_detached_pieces" if pieces else "drop_detached", anchor_min=anchor[0], anchor_max=anchor[1],
                    connectivity=conn, pos=got[0], mrgb=got[1])
        if pieces:
            args.update(piece=got[2], table=got[3])
        return emit(args["call"], args, [("clear", got[0])], [("clear", got[0])])

    def step(kind):
        d = state["depth"]
        if kind in ("set_host", "set_device"):
            pos = set_list()
            pos = pos16(with_duplicates(pos) if kind == "set_device" else pos)
            mrgb = colours(len(pos))
            return emit(kind, {"call": kind[4:], "pos": pos, "mrgb": mrgb}, [("set", pos, mrgb)], [("set", pos, mrgb)])
        if kind in ("clear_host", "clear_device"):
            pos = clear_list()
            pos = pos16(with_duplicates(pos) if kind == "clear_device" else pos)
            return emit(kind, {"call": kind[6:], "pos": pos}, [("clear", pos)], [("clear", pos)])
        if kind == "grid_replace":
            return emit(kind, *grid("replace"))
        if kind == "grid_mask":
            return emit(kind, *grid("set" if rng.random() < 0.5 else "clear"))
        if kind == "depth":
            # up by 1 or 2; past 15 down to the least depth that holds every voxel: a legal shrink (or the depth it has).  So that
            # set_scene_depth shrinks in every sequence, it also does the first time the cube has levels to lose, and one time in
            # two after that (the step after a depth step finds such a cube)
            to, least = d + int(rng.integers(1, 3)), holding_depth(m)
            if to > 15 or (least < d and (not state.get("shrunk") or rng.random() < 0.5)):
                state["shrunk"] = state.get("shrunk", False) or least < d
                to = least
            return emit(kind, {"call": "depth", "to": to}, [], [("depth", to)], depth_after=to)
        if kind == "far_set":
            call = ("host", "device", "grid")[int(rng.integers(3))]
            if call == "grid":
                corner = np.minimum(far_positions(1)[0], 32765)     # the far cell (1, 2, 1) stays an int16 position
                dims, where = (2, 3, 2), [(0, 0, 0), (1, 2, 1)]
                origin = tuple(int(c) for c in corner)
                cells = rng.integers(0, 1 << 31, dims).astype(np.int32)      # junk below bit 31: empty
                for w in where:
                    cells[w] = np.int32(-(1 << 31) + int(rng.integers(0, 1 << 31)))
                pos = pos16([corner + np.array(w) for w in where])
                mrgb = GE.mrgb_of_words([int(cells[w]) for w in where])
                args = {"call": "grid", "cells": cells, "origin": origin, "mode": "set", "grow": True, "pos": pos}
            else:
                pos, mrgb = pos16(far_positions(3)), colours(3)
                args = {"call": call, "pos": pos, "mrgb": mrgb, "grow": True}
            p = pos.astype(np.int64)
            after = max(d, H.cube_depth(p.min(axis=0), p.max(axis=0)))
            twin = ([("depth", after)] if after > d else []) + [("set", pos, mrgb)]
            return emit(kind, args, [("set", pos, mrgb)], twin, depth_after=after, grows=True)
        if kind == "fit":
            left = sorted(p for p in far if p in m)
            clear = pos16(left) if left and rng.random() < 0.5 and len(m) - len(left) >= 2 else pos16([])
            if len(clear):
                far.clear()                  # all of them are gone; one that is set again outside the core cube is added again by emit
            after = dict(m)
            M.apply(after, clear, None)
            to = natural_depth(after)
            return emit(kind, {"call": "fit", "clear": clear}, [("clear", clear)], [("clear", clear), ("fit",)], depth_after=to)
        if kind == "compact":
            return emit(kind, {"call": "compact"}, [], [("compact",)])
        if kind == "mesh":
            name, radius = ("icosphere1", "icosphere2")[int(rng.integers(2))], int(rng.integers(2, 5))
            v, t, surface, inner = shape(name, radius)
            solid = rng.random() < 0.5
            mrgb, fill = colours(1)[0], colours(1)[0]
            cells, bytes_ = union_list(surface, inner, mrgb, fill) if solid else (surface, np.broadcast_to(mrgb & np.array([0x7F, 255, 255, 255], np.uint8), (len(surface), 4)))
            shift, grows = place(cells, overlap=rng.random() < 0.6)
            pos = pos16(cells + shift)
            after = max(d, H.cube_depth(pos.astype(np.int64).min(axis=0), pos.astype(np.int64).max(axis=0)))
            args = {"call": "solid" if solid else "mesh", "verts": (v.astype(np.float64) + shift).astype(np.float32), "tris": t,
                    "mrgb": mrgb, "fill": fill, "grow": grows, "shape": (name, radius), "shift": shift}
            twin = ([("depth", after)] if after > d else []) + [("set", pos, bytes_)]
            return emit(kind, args, [("set", pos, bytes_)], twin, depth_after=after, grows=grows)
        if kind == "carve":
            # the interior lies inside the root cube (its clear is refused otherwise), holds a present voxel and leaves one; the last
            # try is the one-cell cube on a present voxel
            for attempt in range(17):
                name, radius = (("cube", "icosphere1")[int(rng.integers(2))], int(rng.integers(1, 5))) if attempt < 16 else ("cube", 1)
                v, t, _, inner = shape(name, radius)
                shift, outside = place(inner, overlap=True)
                pos = inner + shift
                hit = sum(1 for p in map(tuple, pos.tolist()) if p in m)
                if not outside and hit and len(m) - hit >= 1:
                    break
            else:
                raise AssertionError("no carve that clears a voxel and leaves one")
            pos = pos16(pos)
            args = {"call": "carve", "verts": (v.astype(np.float64) + shift).astype(np.float32), "tris": t, "shape": (name, radius),
                    "shift": shift}
            return emit(kind, args, [("clear", pos)], [("clear", pos)])
        if kind in ("drop_detached", "drop_detached_pieces"):
            return drop(kind == "drop_detached_pieces")
        raise ValueError(kind)

    kinds = circuit(rng)
    counts = [int(c) for c in rng.permutation(BOUNDARY_COUNTS)]
    compacted = False
    for i, kind in enumerate(kinds):
        slots_left = sum(1 for k in kinds[i:] if k in ("set_host", "set_device"))
        if (compacted and counts and kind in ("set_host", "set_device") and room(counts[-1])
                and (rng.random() < 0.5 or slots_left <= len(counts))):
            yield from boundary_pair(counts.pop(), device=kind == "set_device")
        yield step(kind)
        compacted = compacted or kind == "compact"
    if counts and state["depth"] < BOUNDARY_DEPTH:
        yield emit("depth", {"call": "depth", "to": BOUNDARY_DEPTH}, [], [("depth", BOUNDARY_DEPTH)], depth_after=BOUNDARY_DEPTH)
    for k, count in enumerate(counts):
        yield from boundary_pair(count, device=k % 2 == 1)

