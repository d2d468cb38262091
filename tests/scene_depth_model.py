"""The pure-Python model of vxrt_set_scene_depth / vxrt_fit_scene_depth (include/vxrt_scene_depth.h) that the depth tests check the
device against, record for record: the same probe, the same blocks in the same places.  A Scene is the device's
8-byte records (masks | leaf mask << 8, base) and leaf words as vxrt_debug_read_scene returns them, plus the edit bookkeeping the
storage rule depends on: the record / leaf word counts of the build (None until the first edit or depth change)."""
import numpy as np

POPCOUNT = [bin(v).count("1") for v in range(256)]


class Refused(Exception):
    """What the library refuses with VXRT_E_SCENE."""


class Scene:
    def __init__(self, svo, leaves, depth, built=None, live=None):
        self.svo = [[int(m), int(b)] for m, b in np.asarray(svo, np.uint32).reshape(-1, 2).tolist()]
        self.leaves = [int(w) for w in np.asarray(leaves, np.int32).tolist()] or [0]   # api_scene.hip: upload_svo keeps one word
        self.depth = int(depth)
        self.built = built                     # (svo_built, leaf_built) once edited
        self.live = len(self.svo) if live is None else int(live)

    @classmethod
    def build(cls, H, pos, mrgb):
        """What vxrt_set_voxels of the list holds on the device."""
        svo, _, leaves, depth = H.build_records(pos, mrgb)
        return cls(svo, leaves, depth)

    def arrays(self):
        return np.array(self.svo, np.uint32).reshape(-1, 2), np.array(self.leaves, np.int64).astype(np.int32)

    def root_mask(self):
        m = self.svo[0][0]
        return (m >> 8) & 0xFF if self.depth == 0 else m & 0xFF


def _mask(rec, leaf_parent):
    return (rec[0] >> 8) & 0xFF if leaf_parent else rec[0] & 0xFF


def _rank(mask, o):
    return POPCOUNT[mask & ((1 << o) - 1)]


def probe(s):
    """-> (levels the scene can lose, it is the one voxel (-2^t)^3 of depth t = depth - levels): scene_depth.hip's probe."""
    M = s.root_mask()
    if M == 0:
        return s.depth, False
    levels, single = s.depth, False
    for o in range(8):
        if not M >> o & 1:
            continue
        idx, chain, one, n = s.svo[0][1] + _rank(M, o), True, o == 0, 0
        for level in range(1, s.depth + 1):
            if not (chain or one):
                break
            rec = s.svo[idx]
            m = _mask(rec, level == s.depth)
            chain = chain and m == 1 << (o ^ 7)
            if chain:
                n += 1
            else:
                one = one and m == 1
            idx = rec[1]
        levels = min(levels, n)
        if o == 0:
            single = one
    return levels, M == 1 and single


def _change(s, to):
    """The scene at depth `to` (a shrink allowed by the probe): api_scene_depth.hip's change_depth and the two kernels."""
    frm, M = s.depth, s.root_mask()
    if to == frm:
        return
    if s.built is None:
        s.built = (len(s.svo), len(s.leaves))
    m = POPCOUNT[M]
    root = s.svo[0]
    if M and to > frm:
        g = to - frm
        end, lend = len(s.svo), len(s.leaves)
        blocks = g - 1 if frm == 0 else g
        s.svo += [[0, 0] for _ in range(8 + 8 * m * blocks)]
        if frm == 0:
            s.leaves += [0] * (8 * m)
        for o in range(8):
            if not M >> o & 1:
                continue
            r, one = _rank(M, o), 1 << (o ^ 7)
            first, at = end + 8 + 8 * r * blocks, end + r
            for j in range(1, g + 1):
                if j == g and frm == 0:
                    b = lend + 8 * r
                    s.leaves[b] = s.leaves[root[1] + r]
                    s.svo[at] = [one << 8, b]
                else:
                    b = first + 8 * (j - 1)
                    if j == g:
                        s.svo[b] = list(s.svo[root[1] + r])
                    s.svo[at] = [one, b]
                    at = b
        s.svo[0] = [M, end]
        s.live += m * g
    elif M:
        lv = frm - to
        lend = len(s.leaves)
        if to == 0:
            s.leaves += [0] * 8
        for o in range(8):
            if not M >> o & 1:
                continue
            r = _rank(M, o)
            slot = idx = root[1] + r
            for _ in range(lv):
                idx = s.svo[idx][1]
            if to == 0:
                s.leaves[lend + r] = s.leaves[idx]
            else:
                s.svo[slot] = list(s.svo[idx])
        if to == 0:
            s.svo[0] = [M << 8, lend]
        s.live -= m * lv
    s.depth = to


def set_depth(s, depth):
    """vxrt_set_scene_depth on the model (in place); Refused where the library returns VXRT_E_SCENE."""
    assert 0 <= depth <= 15
    if depth < s.depth and s.depth - depth > probe(s)[0]:
        raise Refused(f"a voxel lies outside the root cube of depth {depth}")
    _change(s, depth)
    return s


def fit(s):
    """vxrt_fit_scene_depth on the model (in place) -> the depth."""
    levels, one = probe(s)
    d = s.depth - levels + (1 if one else 0)
    if d > 15:
        raise Refused("the one voxel (-32768)^3")
    _change(s, d)
    return d


def block_owners(s):
    """Every live node's block: [base, base + 8) when it lies at or beyond the build counts (an 8-entry block an edit or a depth
    change allocated, which edit_kernel widens in place), [base, base + popcount) below them; none for a node without children.
    -> True when no two of them share an entry (per array) and no block holds the root record."""
    svo_built, leaf_built = s.built if s.built is not None else (len(s.svo), len(s.leaves))
    taken = ({0}, set())
    level, nodes = 0, [0]
    while nodes:
        leaf_parent = level == s.depth
        nxt = []
        for n in nodes:
            rec = s.svo[n]
            m = _mask(rec, leaf_parent)
            if m == 0:
                continue
            built = leaf_built if leaf_parent else svo_built
            size = 8 if rec[1] >= built else POPCOUNT[m]
            entries = set(range(rec[1], rec[1] + size))
            t = taken[1 if leaf_parent else 0]
            if t & entries:
                return False
            t |= entries
            if not leaf_parent:
                nxt += [rec[1] + _rank(m, o) for o in range(8) if m >> o & 1]
        nodes, level = nxt, level + 1
    return True
