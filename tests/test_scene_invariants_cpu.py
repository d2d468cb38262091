"""CPU: the structural checker of the device records (tests/scene_invariants.py) accepts what the host builder lays out, and the same
trees with every block moved and junk between them, and rejects one hand-made corruption per rule with that rule's message."""
import numpy as np
import pytest

import compact_model as CM
import scene_depth_model as SD
import scene_invariants as SI
from conftest import reference_vox_names
from test_compact_cpu import built


def storage_of(svo, leaves, live=None, spare=0):
    return {"records_live": len(svo) if live is None else live, "records_used": len(svo), "records_capacity": len(svo) + spare,
            "leaves_used": len(leaves), "leaves_capacity": len(leaves) + spare}


def live_records(svo, leaves, depth):
    return len(CM.compact(svo, leaves, depth)[0])


def host_builds(H, scenes):
    for name in reference_vox_names():
        pos, mrgb, _ = scenes.load_scene(name)
        yield name, pos, mrgb
    yield ("startup",) + tuple(H.default_scene_voxels(1))
    yield "empty", np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)


def test_accepts_every_host_build_and_its_damaged_copy(H, scenes):
    rng = np.random.default_rng(8)
    seen = 0
    for name, pos, mrgb in host_builds(H, scenes):
        svo, leaves, depth = built(H, pos, mrgb)
        SI.check(svo, leaves, depth, storage_of(svo, leaves), len(svo))
        SI.check(svo, leaves, depth, storage_of(svo, leaves, spare=5), len(svo), built=(len(svo), len(leaves)))
        moved = CM.damage(svo, leaves, depth, rng)
        live = len(svo)
        SI.check(*moved, depth, storage_of(*moved, live=live), live)
        seen += 1
    assert seen >= 3


def test_accepts_what_depth_changes_leave(H, scenes):
    """grown blocks lie past the build counts, 8 entries each; a shrink back leaves them as holes; depth 0 and back"""
    for name in ("castle", "one", "depth0"):
        if name == "castle":
            pos, mrgb, _ = scenes.load_scene(name)
        elif name == "one":
            pos, mrgb = np.array([[-1, -1, -1]], np.int16), np.array([[1, 2, 3, 4]], np.uint8)
        else:
            pos, mrgb = np.array([[0, 0, 0], [-1, 0, -1]], np.int16), np.array([[1, 2, 3, 4], [0, 9, 8, 7]], np.uint8)
        svo, leaves, depth = built(H, pos, mrgb)
        s = SD.Scene(svo, leaves, depth)
        for to in (depth + 1, depth + 3, 15, depth, depth + 2):
            SD.set_depth(s, to)
            a = s.arrays()
            SI.check(*a, s.depth, storage_of(*a, live=s.live), s.live, built=s.built)
            assert SD.block_owners(s)


@pytest.fixture(scope="module")
def castle(H, scenes):
    pos, mrgb, _ = scenes.load_scene("castle")
    svo, leaves, depth = built(H, pos, mrgb)
    assert depth >= 3
    return svo, leaves, depth


def level_nodes(svo, depth, level):
    """the records of one level, breadth first"""
    idx = np.zeros(1, np.int64)
    for lv in range(level):
        rec = svo[idx].astype(np.int64)
        count = SI.POPCOUNT[rec[:, 0] & 0xFF]
        offset = np.cumsum(count) - count
        idx = np.repeat(rec[:, 1], count) + (np.arange(int(count.sum())) - np.repeat(offset, count))
    return idx


def rejects(rule, svo, leaves, depth, storage=None, nodes=None, built=None):
    storage = storage or storage_of(svo, leaves)
    with pytest.raises(AssertionError) as e:
        SI.check(svo, leaves, depth, storage, storage["records_live"] if nodes is None else nodes, built=built)
    assert str(e.value).startswith(rule + ":"), str(e.value)
    return str(e.value)


def test_rejects_a_block_past_the_records_in_use(castle):
    svo, leaves, depth = castle
    bad = svo.copy()
    n = int(level_nodes(svo, depth, 2)[0])
    bad[n, 1] = len(svo) - 1 if SI.POPCOUNT[bad[n, 0] & 0xFF] > 1 else len(svo)
    assert f"record {n}" in rejects("blocks stay inside storage", bad, leaves, depth)
    bad = svo.copy()
    n = int(level_nodes(svo, depth, depth)[-1])
    bad[n, 1] = len(leaves)
    assert f"record {n}" in rejects("blocks stay inside storage", bad, leaves, depth)


def test_rejects_a_base_pointed_at_a_siblings_block(castle):
    svo, leaves, depth = castle
    nodes = level_nodes(svo, depth, 2)
    a, b = int(nodes[0]), int(nodes[1])
    bad = svo.copy()
    bad[a] = svo[b]                       # equal masks, equal base: the decode sees a valid tree
    msg = rejects("blocks are disjoint", bad, leaves, depth)
    assert f"{a}" in msg and f"{b}" in msg
    parents = level_nodes(svo, depth, depth)
    bad = svo.copy()
    bad[int(parents[0])] = svo[int(parents[1])]
    rejects("blocks are disjoint", bad, leaves, depth)
    bad = svo.copy()                      # across levels: a node of level 2 takes the root's children block; and record 0 itself
    bad[a, 1] = svo[0, 1]
    rejects("blocks are disjoint", bad, leaves, depth)
    bad[a, 1] = 0
    rejects("blocks are disjoint", bad, leaves, depth)


def test_rejects_masks_of_the_wrong_level(castle):
    svo, leaves, depth = castle
    n = int(level_nodes(svo, depth, 1)[0])
    bad = svo.copy()
    bad[n, 0] |= 1 << 8
    assert f"record {n}" in rejects("masks match the level", bad, leaves, depth)
    n = int(level_nodes(svo, depth, depth)[0])
    bad = svo.copy()
    bad[n, 0] |= 1
    assert f"parent {n}" in rejects("masks match the level", bad, leaves, depth)


def test_rejects_an_empty_node(castle):
    svo, leaves, depth = castle
    n = int(level_nodes(svo, depth, 2)[3])
    bad = svo.copy()
    bad[n, 0] = 0
    assert f"record {n}" in rejects("no empty node", bad, leaves, depth)
    n = int(level_nodes(svo, depth, depth)[5])
    bad = svo.copy()
    bad[n, 0] = 0
    assert f"record {n}" in rejects("no empty node", bad, leaves, depth)
    empty = np.array([[0, 1]], np.uint32), np.zeros(1, np.int32)
    for d in (0, 3, 15):
        SI.check(*empty, d, storage_of(*empty), 1)          # the root of the empty scene is the exception


def test_rejects_a_leaf_word_without_its_top_bit(castle):
    svo, leaves, depth = castle
    n = int(level_nodes(svo, depth, depth)[7])
    bad = leaves.copy()
    bad[int(svo[n, 1])] &= 0x7FFFFFFF
    assert f"record {n}" in rejects("leaf words", svo, bad, depth)


def test_rejects_a_live_count_off_by_one(castle):
    svo, leaves, depth = castle
    rejects("live count", svo, leaves, depth, storage_of(svo, leaves, live=len(svo) + 1), nodes=len(svo))
    rejects("live count", svo, leaves, depth, storage_of(svo, leaves, live=len(svo) - 1), nodes=len(svo))
    rejects("live count", svo, leaves, depth, storage_of(svo, leaves), nodes=len(svo) + 1)


def test_rejects_counts_past_the_capacity(castle):
    svo, leaves, depth = castle
    st = storage_of(svo, leaves)
    rejects("bounds", svo, leaves, depth, dict(st, records_capacity=len(svo) - 1))
    rejects("bounds", svo, leaves, depth, dict(st, leaves_capacity=len(leaves) - 1))
    rejects("bounds", svo, leaves, depth, dict(st, records_used=len(svo) + 1, records_capacity=len(svo) + 1))


def test_rejects_a_non_zero_in_the_slack(castle):
    svo, leaves, depth = castle
    st = storage_of(svo, leaves, spare=4)
    long_svo, long_leaves = np.concatenate([svo, np.zeros((4, 2), np.uint32)]), np.concatenate([leaves, np.zeros(4, np.int32)])
    SI.check(long_svo, long_leaves, depth, st, len(svo))
    bad = long_svo.copy()
    bad[len(svo) + 2, 1] = 7
    assert f"record {len(svo) + 2}" in rejects("slack", bad, long_leaves, depth, st)
    bad = long_leaves.copy()
    bad[len(leaves)] = 1
    assert f"leaf word {len(leaves)}" in rejects("slack", long_svo, bad, depth, st)


def test_rejects_an_8_entry_block_moved_by_4(castle):
    """a grown scene: the root's block and every chain node's lie past the build counts, at built + 8k"""
    svo, leaves, depth = castle
    s = SD.Scene(svo, leaves, depth)
    SD.set_depth(s, depth + 2)
    a_svo, a_leaves = s.arrays()
    st = storage_of(a_svo, a_leaves, live=s.live)
    SI.check(a_svo, a_leaves, s.depth, st, s.live, built=s.built)
    chain = int(a_svo[0, 1])                                 # the root's first child: a chain node with one child in a block of 8
    assert a_svo[chain, 1] >= s.built[0]
    bad = np.concatenate([a_svo, np.zeros((8, 2), np.uint32)])
    bad[int(a_svo[chain, 1]) + 4] = bad[int(a_svo[chain, 1])]
    bad[int(a_svo[chain, 1])] = 0
    bad[chain, 1] += 4
    st8 = storage_of(bad, a_leaves, live=s.live)
    SI.check(bad, a_leaves, s.depth, st8, s.live)            # a valid tree for every other rule
    assert f"record {chain}" in rejects("blocks past the build", bad, a_leaves, s.depth, st8, built=s.built)
    # two nodes in one 8-entry frame, their entries apart: the second chain node, which is entry 0 of the first's frame, gets its
    # own child's record as entry 1 of that frame
    frame = int(a_svo[chain, 1])
    bad = a_svo.copy()
    bad[frame + 1] = bad[int(a_svo[frame, 1])]
    bad[frame, 1] = frame + 1
    SI.check(bad, a_leaves, s.depth, st, s.live)
    assert f"record {frame}" in rejects("blocks past the build", bad, a_leaves, s.depth, st, built=s.built)
    # an 8-entry block whose frame passes the records in use: the last chain node's, with the last four records cut off
    short = a_svo[:len(a_svo) - 4]
    st4 = storage_of(short, a_leaves, live=s.live)
    SI.check(short, a_leaves, s.depth, st4, s.live)
    rejects("blocks past the build", short, a_leaves, s.depth, st4, built=s.built)
