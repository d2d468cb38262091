"""The Python model of include/vxrt_grid.h: dense grids <-> voxel lists.  A grid is C order [x][y][z]; cell (i, j, k) is the voxel
at origin + (i, j, k).  PALETTE8 cells are palette indices (0 empty); WORD32 cells are leaf words (bit 31 set = a voxel)."""
import numpy as np

import device_build_model as D
import extract_model as X


def words_of(mrgb):
    """vxrt_set_voxels's leaf word of every (material, r, g, b) -> uint32"""
    return D.leaf_words(mrgb).view(np.uint32)


def mrgb_of(words):
    """the bytes vxrt_set_voxels turns back into the same leaf words"""
    return X.mrgb_of(np.asarray(words).view(np.int32))


def grid_to_list(cells, origin=(0, 0, 0), palette=None):
    """-> (pos int16 [n,3], mrgb uint8 [n,4]) of the occupied cells, in C order of the grid"""
    cells = np.asarray(cells)
    if cells.dtype == np.uint8:
        idx = np.nonzero(cells)
        mrgb = np.asarray(palette, np.uint8).reshape(256, 4)[cells[idx]]
    else:
        w = cells.view(np.uint32)
        idx = np.nonzero(w >> 31)
        mrgb = mrgb_of(w[idx])
    pos = (np.stack(idx, axis=1).astype(np.int64) + np.asarray(origin, np.int64)).astype(np.int16)
    return pos, mrgb.astype(np.uint8).reshape(-1, 4)


def list_to_words(pos, words, origin, dims):
    """Scatter leaf words (uint32) at positions into the box origin + [0, dims) -> int32 grid (0 elsewhere; the last entry wins)."""
    g = np.zeros(tuple(int(d) for d in dims), np.uint32)
    p = np.asarray(pos, np.int64).reshape(-1, 3) - np.asarray(origin, np.int64)
    inside = np.all((p >= 0) & (p < np.asarray(dims, np.int64)), axis=1)
    p = p[inside]
    g[p[:, 0], p[:, 1], p[:, 2]] = np.asarray(words, np.uint32)[inside]
    return g.view(np.int32)


def list_to_grid(pos, mrgb, origin, dims):
    """The WORD32 grid of a voxel list for the box origin + [0, dims)"""
    return list_to_words(pos, words_of(mrgb), origin, dims)


def palette_grid(pos, mrgb, origin, dims):
    """The PALETTE8 grid of a list with at most 255 distinct mrgb -> (uint8 grid, palette [256, 4]), or None with more"""
    mrgb = np.asarray(mrgb, np.uint8).reshape(-1, 4)
    # two mrgb with the same word are the same voxel: key the palette by word
    uniq, inv = np.unique(words_of(mrgb), return_inverse=True)
    if len(uniq) > 255:
        return None
    palette = np.zeros((256, 4), np.uint8)
    palette[1:len(uniq) + 1] = mrgb_of(uniq)
    idx = list_to_words(pos, (inv.reshape(-1) + 1).astype(np.uint32), origin, dims).view(np.uint32)
    return idx.astype(np.uint8), palette


def bounding_box(pos):
    """-> (origin, dims) of the smallest box that holds every position"""
    pos = np.asarray(pos, np.int64).reshape(-1, 3)
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    return tuple(int(v) for v in lo), tuple(int(v) for v in hi - lo + 1)
