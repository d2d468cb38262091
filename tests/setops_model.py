"""The rule of include/vxrt_setops.h in Python (no GPU needed).

Each list is a dict from position to bytes filled in input order, so the last entry of a position wins (transform_model.source_of);
the op is a set expression over the two dicts' keys; the result is sorted by the path key at depth 15 (transform_model.path_key)."""
import numpy as np

from transform_model import path_key, source_of

UNION, INTERSECT, DIFFERENCE, XOR, CHANGED = range(5)
OPS = (UNION, INTERSECT, DIFFERENCE, XOR, CHANGED)
NAMES = ("UNION", "INTERSECT", "DIFFERENCE", "XOR", "CHANGED")


def combine_dicts(a, b, op):
    """Rule 2 on two dicts position -> bytes (or None) -> the result as a dict, unordered."""
    if op == UNION:
        return {**a, **b}                                        # A, then B: last wins
    if op == INTERSECT:
        return {p: a[p] for p in a.keys() & b.keys()}
    if op == DIFFERENCE:
        return {p: a[p] for p in a.keys() - b.keys()}
    if op == XOR:
        return {**{p: a[p] for p in a.keys() - b.keys()}, **{p: b[p] for p in b.keys() - a.keys()}}
    if op == CHANGED:
        return {p: v for p, v in b.items() if p not in a or a[p] != v}
    raise ValueError(op)


def combine(a_pos, a_mrgb, b_pos, b_mrgb, op):
    """Rules 1 to 4 -> (pos int16 [k,3], mrgb uint8 [k,4] or None).  b_mrgb may be None with bytes for INTERSECT and DIFFERENCE."""
    assert op in OPS and (a_mrgb is not None or (b_mrgb is None and op != CHANGED))
    assert a_mrgb is None or b_mrgb is not None or op in (INTERSECT, DIFFERENCE) or len(b_pos) == 0
    out = combine_dicts(source_of(a_pos, a_mrgb), source_of(b_pos, b_mrgb), op)
    keys = sorted(out, key=path_key)
    out_pos = np.array(keys, np.int16).reshape(-1, 3)
    out_mrgb = None if a_mrgb is None else np.array([out[k] for k in keys], np.uint8).reshape(-1, 4)
    return out_pos, out_mrgb


def leaf_word(b):
    """device_build.h: leaf_word_of."""
    return 0x80000000 | (int(b[0]) & 0x7F) << 24 | int(b[1]) << 16 | int(b[2]) << 8 | int(b[3])


def sorted_keys_words(pos, mrgb):
    """What the front of the call hands the merge: the ascending unique path keys of a list and their leaf words."""
    src = source_of(pos, mrgb)
    order = sorted(src, key=path_key)
    return [path_key(p) for p in order], [0 if src[p] is None else leaf_word(src[p]) for p in order]


def combine_keys(a_keys, a_words, b_keys, b_words, op):
    """The op on two ascending unique key lists with words -> [(key, word)] ascending: what the merge must emit."""
    a, b = dict(zip(a_keys, a_words)), dict(zip(b_keys, b_words))
    out = combine_dicts(a, b, op)
    return sorted(out.items())
