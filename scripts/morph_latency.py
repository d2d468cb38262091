"""Latency of vxrt_morph_voxels_device (include/vxrt_morph.h), read against the route a host had before it, on the same machine in
the same run.  Prints one JSON document (profiles/morph/).

Lists: the voxels of menger.vox and monu10.vox, and `--unique` distinct random cells of a 256^3 cube, shuffled, already on the device.
Per list, MORPH_SURFACE and MORPH_DILATE at connectivity 6 and 26, one step:
  `morph`        Context.morph_voxels with cap=None: the counting call and the emitting call
  `morph_tile`   the same with a neighbour looked up in the block's LDS tile before the whole key array (vxrt_debug_morph_tile_lookup:
                 morph_mask_kernel<true> instead of <false>); under `rocprofv3 --kernel-trace --stats` the two kernels' own times are
                 the row that decides between them (profiles/morph/kernel_stats.csv)
  `torch`        the positions with torch: path keys, the c shifted key arrays, cat, sort, unique (DILATE); isin per shift (SURFACE)
The script asserts that all routes give the same positions and that the two lookups give the same bytes.
Host clock around the synchronous call, after one warm-up, median / min / max over the repeats."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_voxel_raytracer_amd import Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.host import MORPH_DILATE, MORPH_SURFACE  # noqa: E402
from pieces_latency import timed  # noqa: E402
from setops_latency import gather16  # noqa: E402
from transform_latency import path_keys  # noqa: E402
from voxelize_latency import DEV  # noqa: E402


def offsets(c):
    """The first c rows of the header's table: by the number of nonzero axes, then by 9 (dx + 1) + 3 (dy + 1) + (dz + 1)."""
    rows = [(dx, dy, dz) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]
    rows.sort(key=lambda o: (sum(1 for d in o if d), 9 * (o[0] + 1) + 3 * (o[1] + 1) + (o[2] + 1)))
    return rows[:c]


def decode(keys):
    return torch.stack([gather16(keys >> 2), gather16(keys >> 1), gather16(keys)], -1).to(torch.int16)


def shifted(upos, o):
    """upos + o -> (path keys, in range)"""
    q = upos + torch.tensor(o, dtype=torch.int64, device=upos.device)
    ok = ((q >= -32768) & (q <= 32767)).all(dim=1)
    return path_keys(torch.where(ok[:, None], q, torch.zeros_like(q))), ok


def torch_dilate(pos, c):
    ukeys = torch.unique(path_keys(pos.to(torch.int64)))
    upos = decode(ukeys).to(torch.int64)
    parts = [ukeys]
    for o in offsets(c):
        keys, ok = shifted(upos, o)
        parts.append(keys[ok])
    return decode(torch.unique(torch.cat(parts)))              # unique sorts: path order


def torch_surface(pos, c):
    ukeys = torch.unique(path_keys(pos.to(torch.int64)))
    upos = decode(ukeys).to(torch.int64)
    inner = torch.ones(len(ukeys), dtype=torch.bool, device=pos.device)
    for o in offsets(c):
        keys, ok = shifted(upos, o)
        inner &= ok & torch.isin(keys, ukeys, assume_unique=False)
    return decode(ukeys[~inner])


def case(ctx, pos, mrgb, repeats):
    out = {"entries": int(len(pos))}
    for name, op, route in (("surface", MORPH_SURFACE, torch_surface), ("dilate", MORPH_DILATE, torch_dilate)):
        for c in (6, 26):
            row = {}
            row["morph"], (m_pos, m_mrgb) = timed(lambda: ctx.morph_voxels(pos, mrgb, op, c), repeats)
            ctx._chk(ctx._L.vxrt_debug_morph_tile_lookup(ctx._h, C.c_uint32(1)), "vxrt_debug_morph_tile_lookup")
            try:
                row["morph_tile"], (p_pos, p_mrgb) = timed(lambda: ctx.morph_voxels(pos, mrgb, op, c), repeats)
            finally:
                ctx._chk(ctx._L.vxrt_debug_morph_tile_lookup(ctx._h, C.c_uint32(0)), "vxrt_debug_morph_tile_lookup")
            row["torch"], r_pos = timed(lambda: route(pos, c), repeats)
            assert torch.equal(m_pos, r_pos), f"{name} at {c}: the two routes disagree"
            assert torch.equal(m_pos, p_pos) and torch.equal(m_mrgb, p_mrgb), f"{name} at {c}: the two lookups disagree"
            row["voxels"] = int(len(m_pos))
            row["morph_over_torch"] = row["morph"]["median_ms"] / row["torch"]["median_ms"]
            row["tile_over_plain"] = row["morph_tile"]["median_ms"] / row["morph"]["median_ms"]
            out[f"{name}_{c}"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    rng = np.random.default_rng(7)
    lists = {}
    for name in ("menger", "monu10"):
        pos, mrgb, _ = scenes.load_scene(name)
        lists[name + ".vox"] = (np.ascontiguousarray(pos, np.int16), np.ascontiguousarray(mrgb, np.uint8))
    side = 256
    cells = rng.choice(side ** 3, args.unique, replace=False)
    cells = np.stack([cells // (side * side), cells // side % side, cells % side], -1) - side // 2
    lists[f"random {args.unique} of {side}^3"] = (np.ascontiguousarray(cells, np.int16), rng.integers(0, 256, (len(cells), 4)).astype(np.uint8))
    result = {}
    with Context(64, 64) as ctx:
        for name, (pos, mrgb) in lists.items():
            result[name] = case(ctx, torch.as_tensor(pos, device=DEV), torch.as_tensor(mrgb, device=DEV), args.repeats)
            print(json.dumps({name: result[name]}), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
