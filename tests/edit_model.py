"""The pure-Python model of vxrt_edit_voxels that the edit tests check the device against: a scene is a dict
{(x, y, z): leaf word}; a set batch overwrites in batch order (so the last entry for a position wins), a clear batch removes and
ignores absent positions.  Plus decoders of the two octree layouts into that dict."""
import numpy as np


def word(mrgb):
    """Leaf word of vxrt_set_voxels (src/context.rs:710-773): 0x80000000 | (material & 0x7f) << 24 | rgb."""
    m, r, g, b = (int(v) for v in mrgb)
    return int(np.int32(np.uint32(0x80000000 | (m & 0x7F) << 24 | r << 16 | g << 8 | b)))


def from_list(pos, mrgb):
    d = {}
    for p, c in zip(np.asarray(pos).tolist(), np.asarray(mrgb).tolist()):
        d[tuple(p)] = word(c)
    return d


def apply(model, pos, mrgb=None):
    """One vxrt_edit_voxels call on the model (in place); mrgb None = clear."""
    pos = np.asarray(pos).reshape(-1, 3).tolist()
    if mrgb is None:
        for p in pos:
            model.pop(tuple(p), None)
    else:
        for p, c in zip(pos, np.asarray(mrgb).reshape(-1, 4).tolist()):
            model[tuple(p)] = word(c)
    return model


def to_list(model):
    """-> (pos int16[n,3], mrgb uint8[n,4]) in a fixed order: what vxrt_set_voxels of the model builds."""
    keys = sorted(model)
    pos = np.array(keys, np.int16).reshape(-1, 3)
    w = np.array([model[k] for k in keys], np.int64).astype(np.uint32)
    mrgb = np.stack([(w >> 24) & 0x7F, (w >> 16) & 0xFF, (w >> 8) & 0xFF, w & 0xFF], axis=1).astype(np.uint8).reshape(-1, 4)
    return pos, mrgb


POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)


def decode_records(svo, leaves, depth):
    """8-byte records (masks | leaf mask << 8, base) + leaf words, as vxrt_debug_read_scene returns them -> dict.  The walk
    follows the pointers from record 0, so it reads the tree whatever the layout (holes included)."""
    svo = np.asarray(svo, np.uint32).reshape(-1, 2)
    idx = np.zeros(1, np.int64)
    u = np.zeros((1, 3), np.int64)
    for level in range(depth + 1):
        rec = svo[idx]
        shift = 8 if level == depth else 0
        masks = (rec[:, 0].astype(np.int64) >> shift) & 0xFF
        nidx, nu = [], []
        for s in range(8):
            has = (masks >> s) & 1 == 1
            if not has.any():
                continue
            rank = POPCOUNT[masks[has] & ((1 << s) - 1)]
            nidx.append(rec[has, 1].astype(np.int64) + rank)
            bits = np.array([(s >> 2) & 1, (s >> 1) & 1, s & 1], np.int64)
            nu.append(u[has] * 2 + bits)
        if not nidx:
            return {}
        idx, u = np.concatenate(nidx), np.concatenate(nu)
        if level == depth:
            coords = u - (1 << depth)
            words = np.asarray(leaves, np.int32)[idx]
            return {tuple(c): int(w) for c, w in zip(coords.tolist(), words.tolist())}
    return {}


def decode_octree_words(words, depth):
    """The reference layout (5-word header, 8 int32 slots per node: > 0 child, < 0 leaf word) -> dict."""
    nodes = np.asarray(words, np.int32)[5:].reshape(-1, 8)
    out = {}
    stack = [(0, 0, (0, 0, 0))]
    while stack:
        node, level, u = stack.pop()
        for s in range(8):
            v = int(nodes[node, s])
            if v == 0:
                continue
            nu = (u[0] * 2 + ((s >> 2) & 1), u[1] * 2 + ((s >> 1) & 1), u[2] * 2 + (s & 1))
            if v < 0:
                assert level == depth
                out[tuple(c - (1 << depth) for c in nu)] = v
            else:
                stack.append((v, level + 1, nu))
    return out
