"""The numpy model of include/vxrt_grid_edit.h: a dense grid written into a box of a scene.  A scene is the edit model's dict
{(x, y, z): leaf word as a signed int32}; a grid is as in tests/grid_model.py (C order [x][y][z], cell (i, j, k) at origin + (i, j, k),
PALETTE8 indices with a palette or WORD32 leaf words).  The call is defined as vxrt_edit_voxels(clears) then vxrt_edit_voxels(sets)
of the two lists this model derives."""
import numpy as np

import grid_model as G

REPLACE, SET, CLEAR = 1, 2, 3
MODES = {"replace": REPLACE, "set": SET, "clear": CLEAR}


class OutsideCube(ValueError):
    """SET or REPLACE with an occupied cell outside the root cube: VXRT_E_SCENE"""


def mode_of(mode):
    return MODES[mode] if isinstance(mode, str) else int(mode)


def grid_words(cells, palette=None):
    """-> int64 array of the grid's leaf words as signed int32 values, 0 for an empty cell"""
    cells = np.asarray(cells)
    if cells.dtype == np.uint8:
        words = np.zeros(256, np.int64)
        words[1:] = G.words_of(np.asarray(palette, np.uint8).reshape(256, 4)[1:]).view(np.int32)
        return words[cells]
    w = cells.view(np.uint32)
    return np.where(w >> 31 == 1, w.view(np.int32).astype(np.int64), 0)


def box_words(model, origin, dims):
    """-> int64 array [dims] of the scene's words in the box origin + [0, dims), 0 where there is no voxel"""
    out = np.zeros(tuple(int(d) for d in dims), np.int64)
    if not model:
        return out
    pos = np.array(list(model.keys()), np.int64).reshape(-1, 3) - np.asarray(origin, np.int64)
    words = np.array(list(model.values()), np.int64)
    inside = np.all((pos >= 0) & (pos < np.asarray(dims, np.int64)), axis=1)
    p = pos[inside]
    out[p[:, 0], p[:, 1], p[:, 2]] = words[inside]
    return out


def in_cube(origin, dims, depth):
    """-> bool array [dims]: the cell lies inside the root cube [-2^depth, 2^depth)^3"""
    h = 1 << depth
    axes = [(np.arange(int(d), dtype=np.int64) + int(o) >= -h) & (np.arange(int(d), dtype=np.int64) + int(o) < h)
            for o, d in zip(origin, dims)]
    return axes[0][:, None, None] & axes[1][None, :, None] & axes[2][None, None, :]


def edit_lists(model, cells, origin, mode, depth, palette=None):
    """-> (clears: int16 [n, 3] positions, sets: int16 [m, 3] positions, set words: int64 [m], the edited dict).  Raises OutsideCube
    for SET / REPLACE with an occupied cell outside the root cube."""
    mode = mode_of(mode)
    cells = np.asarray(cells)
    g = grid_words(cells, palette)
    dims = cells.shape
    inside = in_cube(origin, dims, depth)
    occ = g != 0
    if mode != CLEAR and np.any(occ & ~inside):
        raise OutsideCube("an occupied cell lies outside the root cube")
    s = box_words(model, origin, dims)
    if mode == REPLACE:
        clear, sets = inside & ~occ & (s != 0), inside & occ & (s != g)
    elif mode == SET:
        clear, sets = np.zeros_like(occ), inside & occ & (s != g)
    else:
        clear, sets = inside & occ & (s != 0), np.zeros_like(occ)
    o = np.asarray(origin, np.int64)
    cpos = (np.argwhere(clear) + o).astype(np.int16).reshape(-1, 3)
    spos = (np.argwhere(sets) + o).astype(np.int16).reshape(-1, 3)
    swords = g[sets]
    out = dict(model)
    for p in cpos.tolist():
        out.pop(tuple(p), None)
    for p, w in zip(spos.tolist(), swords.tolist()):
        out[tuple(p)] = int(w)
    return cpos, spos, swords, out


def mrgb_of_words(words):
    """the (material, r, g, b) bytes whose vxrt_edit_voxels leaf words are `words` (signed or unsigned int32 values)"""
    return G.mrgb_of(np.asarray(words, np.int64).astype(np.uint32)).reshape(-1, 4)


def box_of(model, origin, dims):
    """the model's box as vxrt_get_voxel_grid writes it: int32 leaf words, 0 for empty cells and cells outside the root cube"""
    return box_words(model, origin, dims).astype(np.int32)
