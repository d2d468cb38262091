"""The Python model of vxrt_get_voxels (include/vxrt_extract.h) that the extract tests check the device against: the octree path
order of a voxel list, a pointer-following decode of the device records restricted to a box, and the Menger sponge's membership and
count (config 5's scene) computed from its base-3 digits."""
import numpy as np

import edit_model as M


def path_key(pos, depth):
    """Octree path key of every position (vxrt_extract.h "Order"): with u = p + 2^depth, digit k (k = depth .. 0, the root's first)
    is  (bit k of u.x) << 2 | (bit k of u.y) << 1 | (bit k of u.z),  and key = sum of digit_k << 3k."""
    u = np.asarray(pos, np.int64).reshape(-1, 3) + (1 << depth)
    key = np.zeros(len(u), np.int64)
    for k in range(depth + 1):
        digit = ((u[:, 0] >> k) & 1) << 2 | ((u[:, 1] >> k) & 1) << 1 | ((u[:, 2] >> k) & 1)
        key |= digit << (3 * k)
    return key


def path_order(pos, depth):
    """Indices that put a list of distinct positions in ascending path order."""
    return np.argsort(path_key(pos, depth), kind="stable")


def mrgb_of(words):
    """Leaf words -> (material & 0x7f, r, g, b) bytes: what vxrt_set_voxels turns back into the same words."""
    w = np.asarray(words, np.int64).astype(np.uint32).reshape(-1)
    return np.stack([(w >> 24) & 0x7F, (w >> 16) & 0xFF, (w >> 8) & 0xFF, w & 0xFF], axis=1).astype(np.uint8).reshape(-1, 4)


def ordered_list(model, depth):
    """A model dict {(x, y, z): word} -> (pos int16[n,3], mrgb uint8[n,4]) in path order: what vxrt_get_voxels returns for it."""
    keys = sorted(model)
    pos = np.array(keys, np.int64).reshape(-1, 3)
    words = np.array([model[k] for k in keys], np.int64)
    order = path_order(pos, depth)
    return pos[order].astype(np.int16), mrgb_of(words[order])


def input_list(pos, mrgb, depth):
    """A vxrt_set_voxels input (duplicates: the last entry wins) -> its voxels in path order."""
    return ordered_list(M.from_list(pos, mrgb), depth)


def in_box(pos, box):
    """Which positions lie in the half-open box (lo, hi); box None = all."""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    if box is None:
        return np.ones(len(pos), bool)
    lo, hi = (np.asarray(b, np.int64).reshape(1, 3) for b in box)
    return np.all((pos >= lo) & (pos < hi), axis=1)


def decode_records_box(svo, leaves, depth, box=None):
    """8-byte records (masks | leaf mask << 8, base) + leaf words, as vxrt_debug_read_scene returns them, -> (pos int16[n,3],
    mrgb uint8[n,4]) of the voxels in the half-open box (lo, hi) (None = all), in path order.  The walk follows the pointers from
    record 0 level by level and descends only into children whose cubes meet the box: whatever the layout, it never scans the arrays."""
    svo = np.asarray(svo, np.uint32).reshape(-1, 2)
    half = 1 << depth
    if box is None:
        lo, hi = np.zeros(3, np.int64), np.full(3, 2 * half, np.int64)
    else:
        lo = np.clip(np.asarray(box[0], np.int64) + half, 0, 2 * half)
        hi = np.clip(np.asarray(box[1], np.int64) + half, 0, 2 * half)
    empty = (np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8))
    if len(svo) == 0 or np.any(lo >= hi):
        return empty
    slots = np.arange(8, dtype=np.int64)
    bits = np.stack([(slots >> 2) & 1, (slots >> 1) & 1, slots & 1], axis=1)       # [8, 3]
    idx = np.zeros(1, np.int64)
    u = np.zeros((1, 3), np.int64)
    for level in range(depth + 1):
        rec = svo[idx]
        leaf = level == depth
        mask = (rec[:, 0].astype(np.int64) >> (8 if leaf else 0)) & 0xFF
        shift = depth - level
        child = u[:, None, :] * 2 + bits[None, :, :]                                # [n, 8, 3]
        meets = np.all(((child << shift) < hi) & (((child + 1) << shift) > lo), axis=2)
        keep = ((mask[:, None] >> slots[None, :]) & 1 == 1) & meets                   # [n, 8]: node-major, then slot: path order
        node, slot = np.nonzero(keep)
        if len(node) == 0:
            return empty
        target = rec[node, 1].astype(np.int64) + M.POPCOUNT[mask[node] & ((1 << slot) - 1)]
        u = child[node, slot]
        if leaf:
            words = np.asarray(leaves, np.int32)[target]
            return (u - half).astype(np.int16), mrgb_of(words)
        idx = target
    return empty


def menger_solid(level, pos):
    """Config 5's membership rule (scene_host.cpp: menger_solid) on voxel cells (x, y, z) >= 0 of the unclipped sponge: solid unless,
    at some base-3 digit position, two or more coordinates have digit 1."""
    p = np.asarray(pos, np.int64).reshape(-1, 3).copy()
    solid = np.all((p >= 0) & (p < 3 ** level), axis=1)
    for _ in range(level):
        solid &= np.sum(p % 3 == 1, axis=1) < 2
        p //= 3
    return solid


def menger_count(level, clip):
    """The number of solid cells of the level-`level` sponge in [0, clip)^3, by a digit DP over the base-3 digits from the most
    significant: the state is which axes are still equal to clip's prefix (those may not exceed clip's next digit)."""
    side = 3 ** level
    bound = min(clip, side)
    if bound == side:
        return 20 ** level
    digits = [(bound // 3 ** k) % 3 for k in range(level - 1, -1, -1)]   # bound's digits, most significant first
    states = {(True, True, True): 1}
    for d in digits:
        nxt = {}
        for tight, ways in states.items():
            for dx in range(3):
                for dy in range(3):
                    for dz in range(3):
                        if (dx == 1) + (dy == 1) + (dz == 1) >= 2:
                            continue
                        t = []
                        ok = True
                        for ti, di in zip(tight, (dx, dy, dz)):
                            if ti and di > d:
                                ok = False
                                break
                            t.append(ti and di == d)
                        if ok:
                            nxt[tuple(t)] = nxt.get(tuple(t), 0) + ways
        states = nxt
    # cells equal to the bound on some axis are not < bound
    return sum(w for t, w in states.items() if not any(t))
