"""A structural checker of the device records of an editable scene: the storage rule of DESIGN.md §9, §14 and §16 as assertions on
the raw arrays, where edit_model.decode_records only follows the pointers.  Numpy, level by level from record 0, as decode_records.

check() raises AssertionError("<rule>: ...") naming the first violated rule and the record index.  The rules, in the order they run:

  bounds            records_used <= records_capacity and leaves_used <= leaves_capacity, and the read-back holds at least the used
                    counts.
  slack             everything the read-back holds at or past records_used / leaves_used is zero.  vxrt_debug_read_scene stops at the
                    used counts (api_scene.hip copies svo_count records and leaf_count words), so on the device this rule has nothing
                    to look at: it only judges arrays a caller hands in longer than the counts, as the CPU tests do.  The slack of
                    the allocation itself (grow_to's memset) cannot be read back and is not checked.
  masks match the level   an interior record (level < depth) has leaf mask 0, a leaf parent has child mask 0.
  no empty node     no reachable record has mask 0, except the root of the empty scene.
  blocks stay inside storage   a reachable node's block [base, base + popcount(mask)) lies inside [0, records_used), or inside
                    [0, leaves_used) for a leaf parent's words.
  blocks past the build   with built = (svo_built, leaf_built): a block whose base is at or past the build count starts at built + 8k
                    and owns the whole frame [base, base + 8), which lies inside the used count too.  This holds as the code stands,
                    without a restriction: edit_kernel hands out new blocks at svo_end + 8 * rank and advances by 8 * total
                    (edit.hip), depth_grow places the root's block at svo_end and one 8-entry block per chain node after it, a shrink
                    to depth 0 takes 8 leaf words at leaf_end (api_scene_depth.hip: svo_add, leaf_add are multiples of 8), a shrink
                    otherwise writes into the root's block only, and both take the build counts (the counts in use at the first edit
                    or depth change) before they allocate.  A compaction leaves a fresh scene (`edited` false, used = live), so the
                    next edit or depth change takes the counts anew: the caller passes the compacted counts as `built` from then on.
                    A node that moved records (a shrink copies a record into the root's block) keeps that record's base, and so its
                    block.  built None skips the rule.
  blocks are disjoint   the blocks of distinct reachable nodes share no entry, at any level or across levels, and record 0 belongs
                    to no block.  A block past the build counts counts with its whole 8-entry frame (edit_kernel widens it in
                    place), so two nodes in one frame are found even while their entries do not overlap.
  leaf words        every reachable leaf word has bit 31 set.  Bits 24-30 are the material & 0x7f: every value of those seven bits
                    is one, so the structure has nothing more to say about them (the decoded dict is compared with the model's).
  live count        the number of reachable records equals records_live and octree_nodes.
"""
import numpy as np

POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)


def _first(bad):
    return int(np.flatnonzero(bad)[0])


def _disjoint(base, size, owner, what, reserved):
    """blocks [base, base + size) owned by records `owner`: none below `reserved`, no two sharing an entry"""
    if len(base) == 0:
        return
    low = base < reserved
    assert not low.any(), f"blocks are disjoint: the block of record {int(owner[_first(low)])} holds {what} {int(base[_first(low)])}, the root's own"
    order = np.argsort(base, kind="stable")
    b, s, o = base[order], size[order], owner[order]
    clash = b[:-1] + s[:-1] > b[1:]
    if clash.any():
        i = _first(clash)
        raise AssertionError(f"blocks are disjoint: the blocks of records {int(o[i])} and {int(o[i + 1])} share {what} {int(b[i + 1])}")


def check(svo, leaves, depth, storage, octree_nodes, built=None):
    """svo, leaves: read_scene(); depth: scene_depth; storage: scene_storage(); octree_nodes: stats().octree_nodes; built: the
    (record, leaf word) counts of the build, tracked by the caller (see the module docstring), or None."""
    svo = np.asarray(svo, np.uint32).reshape(-1, 2)
    leaves = np.asarray(leaves, np.int32).reshape(-1)
    used, lused = int(storage["records_used"]), int(storage["leaves_used"])
    assert used <= int(storage["records_capacity"]), f"bounds: {used} records in use, {storage['records_capacity']} allocated"
    assert lused <= int(storage["leaves_capacity"]), f"bounds: {lused} leaf words in use, {storage['leaves_capacity']} allocated"
    assert 1 <= used <= len(svo), f"bounds: {used} records in use, {len(svo)} read back"
    assert lused <= len(leaves), f"bounds: {lused} leaf words in use, {len(leaves)} read back"
    tail = np.any(svo[used:] != 0, axis=1)
    assert not tail.any(), f"slack: record {used + _first(tail)} past the {used} in use is not zero"
    ltail = leaves[lused:] != 0
    assert not ltail.any(), f"slack: leaf word {lused + _first(ltail)} past the {lused} in use is not zero"

    rec_blocks, reachable = [], 1
    idx = np.zeros(1, np.int64)
    for level in range(depth + 1):
        leaf_parents = level == depth
        rec = svo[idx].astype(np.int64)
        child, leaf, base = rec[:, 0] & 0xFF, (rec[:, 0] >> 8) & 0xFF, rec[:, 1]
        if leaf_parents:
            bad, mask = child != 0, leaf
            assert not bad.any(), f"masks match the level: leaf parent {int(idx[_first(bad)])} (level {level}) has a child mask"
        else:
            bad, mask = leaf != 0, child
            assert not bad.any(), f"masks match the level: interior record {int(idx[_first(bad)])} (level {level}) has a leaf mask"
        empty = mask == 0
        if level == 0 and empty[0]:
            break                                   # the empty scene: the root alone, whatever its depth
        assert not empty.any(), f"no empty node: record {int(idx[_first(empty)])} (level {level}) has mask 0"
        count = POPCOUNT[mask]
        end, what = (lused, "leaf word") if leaf_parents else (used, "record")
        out = base + count > end
        assert not out.any(), (f"blocks stay inside storage: the block [{int(base[_first(out)])}, +{int(count[_first(out)])}) of record "
                               f"{int(idx[_first(out)])} passes the {end} {what}s in use")
        size = count
        if built is not None:
            b0 = int(built[1 if leaf_parents else 0])
            past = base >= b0
            off = past & ((base - b0) % 8 != 0)
            assert not off.any(), (f"blocks past the build: the block of record {int(idx[_first(off)])} starts at {what} "
                                   f"{int(base[_first(off)])}, not at {b0} + 8k")
            over = past & (base + 8 > end)
            assert not over.any(), (f"blocks past the build: the 8-entry block of record {int(idx[_first(over)])} at {what} "
                                    f"{int(base[_first(over)])} passes the {end} in use")
            size = np.where(past, 8, count)
        if leaf_parents:
            _disjoint(base, size, idx, what, 0)
            offset = np.cumsum(count) - count
            words = leaves[np.repeat(base, count) + (np.arange(int(count.sum()), dtype=np.int64) - np.repeat(offset, count))]
            bad = words >= 0
            if bad.any():
                i = _first(bad)
                node = int(idx[np.searchsorted(offset, i, side="right") - 1])
                raise AssertionError(f"leaf words: a leaf word of record {node} has bit 31 clear ({int(words[i]) & 0xFFFFFFFF:#010x})")
        else:
            rec_blocks.append((base, size, idx))
            _disjoint(*(np.concatenate([b[k] for b in rec_blocks]) for k in range(3)), what, 1)   # before the next level is walked
            offset = np.cumsum(count) - count
            idx = np.repeat(base, count) + (np.arange(int(count.sum()), dtype=np.int64) - np.repeat(offset, count))
            reachable += len(idx)
    live = int(storage["records_live"])
    assert reachable == live, f"live count: {reachable} records are reachable from record 0, records_live is {live}"
    assert reachable == int(octree_nodes), f"live count: {reachable} records are reachable from record 0, octree_nodes is {int(octree_nodes)}"
