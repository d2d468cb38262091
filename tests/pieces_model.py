"""Rules 6 to 9 of include/vxrt_pieces.h in numpy and pure Python, on top of components_model.py's rules 1 to 5.

    component_table(pos, connectivity) -> (label uint32 [n], id uint32 [n], table)
    detached_pieces(voxels, anchor_min, anchor_max, connectivity, min_voxels, max_voxels) -> (pos, mrgb, piece, table)

table is a numpy record array of dtype PIECE, the layout of vxrt_piece (48 bytes), `reserved` 0.  Nothing here follows the library's
pipeline: a component's distinct positions are collected in a Python set and counted, bounded and summed in Python integers."""
import numpy as np

import components_model as K

PIECE = np.dtype([("first", "<u4"), ("voxels", "<u4"), ("min", "<i2", (3,)), ("max", "<i2", (3,)), ("reserved", "<u4"), ("sum", "<i8", (3,))])
assert PIECE.itemsize == 48 and PIECE.fields["sum"][1] == 24
FIELDS = ("first", "voxels", "min", "max", "sum")
EVERY = 0xFFFFFFFF


def _row(first, cells):
    """cells: a set of (x, y, z) -> one record"""
    row = np.zeros((), PIECE)
    row["first"], row["voxels"] = first, len(cells)
    for ax in range(3):
        values = [c[ax] for c in cells]
        row["min"][ax], row["max"][ax], row["sum"][ax] = min(values), max(values), sum(values)
    return row


def component_table(pos, connectivity):
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    label, count = K.label(pos, connectivity)
    labels = sorted(set(label.tolist()))                    # rule 6: numbered by ascending label
    assert len(labels) == count
    number = {first: c for c, first in enumerate(labels)}
    ids = np.array([number[first] for first in label.tolist()], np.uint32).reshape(-1)
    cells = [set() for _ in labels]
    for p, c in zip(pos.tolist(), ids.tolist()):
        cells[c].add(tuple(p))                              # rule 8: a position counts once
    table = np.zeros(count, PIECE)
    for c, first in enumerate(labels):
        table[c] = _row(first, cells[c])                    # rule 7
    return label, ids, table


def detached_pieces(voxels, anchor_min, anchor_max, connectivity, min_voxels=0, max_voxels=EVERY):
    """voxels: {(x, y, z): (m, r, g, b)} -> (pos int16 [k, 3], mrgb uint8 [k, 4], piece uint32 [k], table PIECE [pieces]): the
    components with no voxel in the half-open anchor box and min_voxels <= size <= max_voxels, their voxels in ascending path
    order, numbered by their first voxel in that order; a record's `first` is that voxel's index in the returned list"""
    cells = list(voxels)
    sets, index = K.classes_of(cells, connectivity)
    lo, hi = [int(v) for v in anchor_min], [int(v) for v in anchor_max]
    members = {}
    for c, i in index.items():
        members.setdefault(sets.find(i), set()).add(c)
    held = {sets.find(i) for c, i in index.items() if all(lo[k] <= c[k] < hi[k] for k in range(3))}
    chosen = {r for r, m in members.items() if r not in held and min_voxels <= len(m) <= max_voxels}
    loose = [c for c, i in index.items() if sets.find(i) in chosen]
    if not loose:
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8), np.zeros(0, np.uint32), np.zeros(0, PIECE)
    pos = np.array(loose, np.int64)
    pos = pos[np.argsort(K.path_keys(pos), kind="stable")]
    mrgb = np.array([voxels[tuple(p)] for p in pos.tolist()], np.uint8).reshape(-1, 4)
    number, firsts, piece = {}, [], []
    for at, p in enumerate(pos.tolist()):
        r = sets.find(index[tuple(p)])
        if r not in number:
            number[r] = len(firsts)
            firsts.append(at)
        piece.append(number[r])
    table = np.zeros(len(firsts), PIECE)
    for r, c in number.items():
        table[c] = _row(firsts[c], members[r])
    return pos.astype(np.int16), mrgb, np.array(piece, np.uint32), table
