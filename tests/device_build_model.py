"""The Python model of vxrt_set_voxels_device (include/vxrt_device_scene.h): the records and leaf words the host builder makes
(flatten_svo(build_octree(list))), restated the way the device builds them — sort by path key, keep the last entry of every key,
then the node levels bottom-up as runs of key >> 3."""
import numpy as np

import extract_model as X


def _ceil_log2(v):
    """u16::next_power_of_two().trailing_zeros()"""
    bits = 0
    while (1 << bits) < v:
        bits += 1
    return bits


def depth_of(pos):
    """build_octree's depth rule (scene_host.cpp): |min| and |max| + 1 of all coordinates, each masked to 16 bits, rounded up to
    a power of two; None for depth > 15 (VXRT_E_SCENE)."""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    if len(pos) == 0:
        return 0
    lo, hi = int(pos.min()), int(pos.max())
    d = max(_ceil_log2(abs(lo) & 0xFFFF), _ceil_log2((abs(hi) + 1) & 0xFFFF))
    return None if d > 15 else d


def leaf_words(mrgb):
    m = np.asarray(mrgb, np.uint8).reshape(-1, 4).astype(np.uint32)
    return (np.uint32(0x80000000) | (m[:, 0] & 0x7F) << 24 | m[:, 1] << 16 | m[:, 2] << 8 | m[:, 3]).view(np.int32)


def build(pos, mrgb):
    """-> (svo uint32[n,2] = masks, base; leaves int32[k]; depth), as H.build_records returns them (the empty list: the root
    {0, 1} and no leaf word)."""
    pos = np.asarray(pos, np.int16).reshape(-1, 3)
    mrgb = np.asarray(mrgb, np.uint8).reshape(-1, 4)
    if len(pos) == 0:
        return np.array([[0, 1]], np.uint32), np.zeros(0, np.int32), 0
    depth = depth_of(pos)
    if depth is None:
        raise ValueError("octree depth > 15")
    key = X.path_key(pos, depth)
    order = np.argsort(key, kind="stable")
    key, words = key[order], leaf_words(mrgb)[order]
    last = np.r_[key[1:] != key[:-1], True]                  # the last entry of every key wins
    below, leaves = key[last], words[last]
    levels = []                                               # bottom-up: (masks, first index in the level below)
    for j in range(1, depth + 2):
        parent = below >> 3
        first = np.flatnonzero(np.r_[True, parent[1:] != parent[:-1]])
        mask = np.bitwise_or.reduceat(np.left_shift(1, below & 7), first)
        levels.append((mask if j > 1 else mask << 8, first))
        below = parent[first]
    assert len(below) == 1 and below[0] == 0
    sizes = [len(m) for m, _ in levels]
    start = np.cumsum([0] + sizes[::-1])[:-1][::-1]           # top-down start of every level, listed bottom-up
    svo = np.zeros((sum(sizes), 2), np.uint32)
    for j, (mask, first) in enumerate(levels):
        base = first if j == 0 else first + start[j - 1]
        svo[start[j]:start[j] + len(mask)] = np.stack([mask, base], axis=1)
    return svo, leaves.astype(np.int32), depth


def record_count(pos):
    """The number of records of the list's tree (without materialising them)."""
    pos = np.asarray(pos, np.int16).reshape(-1, 3)
    if len(pos) == 0:
        return 1
    depth = depth_of(pos)
    below = np.unique(X.path_key(pos, depth))
    total = 0
    for _ in range(depth + 1):
        below = np.unique(below >> 3)
        total += len(below)
    return total
