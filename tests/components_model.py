"""The rule of include/vxrt_components.h in numpy and pure Python: a dict of positions and a union-find over it.

    label(pos, connectivity) -> (label uint32 [n], n_components)     label[i] = the least index of an entry in i's component
    detached(voxels, anchor_min, anchor_max, connectivity) -> the positions of a voxel dict {(x, y, z): bytes} whose component
                                                              holds no voxel in the half-open anchor box, in path order

Nothing here follows the library's pipeline: no keys, no sort, no neighbour search by bisection; a position's neighbours are looked up
in a dict, offset by offset, and the classes are merged by size with full path compression."""
import itertools

import numpy as np

CONNECTIVITIES = (6, 18, 26)
LO, HI = -32768, 32767          # coordinates are int16 and do not wrap


def offsets(connectivity):
    """the nonzero offsets with |d| <= 1 per axis that differ on at most 1, 2 or 3 axes: 6, 18 or 26 of them"""
    axes = {6: 1, 18: 2, 26: 3}[connectivity]
    out = [d for d in itertools.product((-1, 0, 1), repeat=3) if 0 < sum(c != 0 for c in d) <= axes]
    assert len(out) == connectivity
    return out


class Classes:
    def __init__(self, n):
        self.parent = list(range(n))
        self.size = [1] * n

    def find(self, a):
        root = a
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[a] != root:
            self.parent[a], a = root, self.parent[a]
        return root

    def join(self, a, b):
        a, b = self.find(a), self.find(b)
        if a == b:
            return
        if self.size[a] < self.size[b]:
            a, b = b, a
        self.parent[b] = a
        self.size[a] += self.size[b]


def classes_of(cells, connectivity):
    """cells: a list of distinct (x, y, z) -> (Classes over their indices, {cell: index})"""
    index = {c: i for i, c in enumerate(cells)}
    assert len(index) == len(cells)
    # every cell is an int16 position, so a neighbour beyond int16 is in no list: there is no such voxel, and in Python integers
    # nothing wraps around to one
    assert all(LO <= v <= HI for c in cells for v in c)
    sets = Classes(len(cells))
    offs = [d for d in offsets(connectivity) if d > (0, 0, 0)]      # adjacency is symmetric: one of d and -d finds every pair
    assert 2 * len(offs) == connectivity
    for c, i in index.items():
        for d in offs:
            j = index.get((c[0] + d[0], c[1] + d[1], c[2] + d[2]))
            if j is not None:
                sets.join(i, j)
    return sets, index


def label(pos, connectivity):
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    entries = [tuple(p) for p in pos.tolist()]
    cells = list(dict.fromkeys(entries))          # each position once (entries at one position are adjacent)
    sets, index = classes_of(cells, connectivity)
    least = {}
    for i, e in enumerate(entries):
        least.setdefault(sets.find(index[e]), i)  # the first entry met is the least index
    out = np.array([least[sets.find(index[e])] for e in entries], np.uint32).reshape(-1)
    return out, int((out == np.arange(len(out))).sum())


def path_keys(pos, depth=15):
    """the order of vxrt_get_voxels (include/vxrt_extract.h): u = p + 2^depth, bits interleaved x, y, z from the top"""
    u = np.asarray(pos, np.int64).reshape(-1, 3) + (1 << depth)
    keys = np.zeros(len(u), np.int64)
    for k in range(depth + 1):
        keys |= (((u[:, 0] >> k) & 1) << 2 | ((u[:, 1] >> k) & 1) << 1 | ((u[:, 2] >> k) & 1)) << (3 * k)
    return keys


def detached(voxels, anchor_min, anchor_max, connectivity):
    """-> (pos int16 [k, 3], mrgb uint8 [k, 4]) of the voxel dict's detached voxels, in ascending path order"""
    cells = list(voxels)
    sets, index = classes_of(cells, connectivity)
    lo, hi = [int(v) for v in anchor_min], [int(v) for v in anchor_max]
    held = {sets.find(i) for c, i in index.items() if all(lo[k] <= c[k] < hi[k] for k in range(3))}
    loose = [c for c, i in index.items() if sets.find(i) not in held]
    if not loose:
        return np.zeros((0, 3), np.int16), np.zeros((0, 4), np.uint8)
    pos = np.array(loose, np.int64)
    order = np.argsort(path_keys(pos), kind="stable")
    pos = pos[order]
    mrgb = np.array([voxels[tuple(p)] for p in pos.tolist()], np.uint8).reshape(-1, 4)
    return pos.astype(np.int16), mrgb
