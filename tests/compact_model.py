"""The numpy model of vxrt_compact_scene (include/vxrt_compact.h) that the compaction tests check the device against, byte for byte:
8-byte records (masks | leaf mask << 8, base) and leaf words in ANY valid layout — the build's, the holes and 8-entry blocks edits and
depth changes leave, blocks in any order — -> the arrays of a fresh build of the same tree (api_scene.hip: flatten_svo): records
breadth first and level by level, children in their parents' order with slots ascending, every block tight, a leaf parent's base the
running count of leaf words.  The walk follows the pointers from record 0, one level at a time."""
import numpy as np

POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)


def compact(svo, leaves, depth):
    """-> (svo uint32[n, 2], leaves int32[k]) as vxrt_debug_read_scene returns them after vxrt_compact_scene."""
    svo = np.asarray(svo, np.uint32).reshape(-1, 2)
    leaves = np.asarray(leaves, np.int32)
    if len(svo) == 0 or int(svo[0, 0]) & 0xFFFF == 0:
        return np.array([[0, 1]], np.uint32), np.zeros(1, np.int32)     # what vxrt_set_voxels holds for an empty list
    out = []
    idx = np.zeros(1, np.int64)      # this level's nodes, breadth first: their records in the given layout
    start = 0                        # ... and where the level starts in the new one
    for level in range(depth + 1):
        rec = svo[idx]
        leaf_parents = level == depth
        masks = ((rec[:, 0].astype(np.int64) >> 8) if leaf_parents else rec[:, 0].astype(np.int64)) & 0xFF
        count = POPCOUNT[masks]
        offset = np.cumsum(count) - count
        below = start + len(idx)
        base = offset if leaf_parents else below + offset
        out.append(np.stack([rec[:, 0].astype(np.int64), base], axis=1))
        # slot j of a node lies at base + j in the given layout, whatever block that is
        total = int(count.sum())
        first = np.repeat(rec[:, 1].astype(np.int64), count)
        child = first + (np.arange(total, dtype=np.int64) - np.repeat(offset, count))
        if leaf_parents:
            assert total > 0, "a tree with voxels has leaf words"
            return np.concatenate(out).astype(np.uint32), leaves[child].copy()
        assert total > 0, "an inner node has a child"
        idx, start = child, below
    raise AssertionError("unreachable")


def damage(svo, leaves, depth, rng, slack=3):
    """The same tree with every sibling block moved: the blocks in a seeded random order, with up to `slack` unused entries (filled
    with junk) between them, the leaf blocks likewise.  Record 0 stays the root.  -> (svo, leaves)."""
    svo = np.asarray(svo, np.uint32).reshape(-1, 2)
    leaves = np.asarray(leaves, np.int32)
    if int(svo[0, 0]) & 0xFFFF == 0:
        return svo.copy(), leaves.copy()
    # the live nodes, level by level, with the index of each node's parent
    levels, idx = [], np.zeros(1, np.int64)
    for level in range(depth + 1):
        rec = svo[idx]
        masks = ((rec[:, 0].astype(np.int64) >> 8) if level == depth else rec[:, 0].astype(np.int64)) & 0xFF
        count = POPCOUNT[masks]
        levels.append((idx, count))
        if level < depth:
            offset = np.cumsum(count) - count
            idx = np.repeat(rec[:, 1].astype(np.int64), count) + (np.arange(int(count.sum())) - np.repeat(offset, count))
    new_svo = [[int(svo[0, 0]), 0]]     # grows as blocks are placed
    new_leaves = []
    where = np.zeros(1, np.int64)       # new index of every node of the current level
    for level, (idx, count) in enumerate(levels):
        order = rng.permutation(len(idx))
        target = new_leaves if level == depth else new_svo
        base = np.zeros(len(idx), np.int64)
        for n in order.tolist():
            for _ in range(int(rng.integers(0, slack + 1))):
                target.append(int(rng.integers(1, 1 << 31)) if level == depth else [int(rng.integers(0, 1 << 16)), int(rng.integers(0, 1 << 31))])
            base[n] = len(target)
            src = int(svo[idx[n], 1])
            for j in range(int(count[n])):
                target.append(int(leaves[src + j]) if level == depth else [int(svo[src + j, 0]), 0])
        for n in range(len(idx)):
            new_svo[int(where[n])][1] = int(base[n])
        if level < depth:
            offset = np.cumsum(count) - count
            where = np.repeat(base, count) + (np.arange(int(count.sum())) - np.repeat(offset, count))
    return np.array(new_svo, np.uint32).reshape(-1, 2), np.array(new_leaves, np.int64).astype(np.int32)
