"""Latency of vxrt_combine_voxels_device (include/vxrt_setops.h), read against the route a host had before it, on the same machine in
the same run.  Prints one JSON document (profiles/setops/).

Two lists of about `--unique` distinct voxels each, half of them in common, random cells of a cube, shuffled, already on the device.
  `union`            Context.combine_voxels(LIST_UNION): the counting call and the emitting call
  `count_intersect`  Context.count_common: the counting call alone (the collision test)
  `torch_union`      the same bytes with torch: path keys, cat, a stable sort, the last entry of each key, decode
  `torch_intersect`  the count with torch: the two lists' unique keys, cat, sort, unique_consecutive with counts, a mask, a sum
The script asserts that both routes give the same bytes and the same count.
Host clock around the synchronous call, after one warm-up, median / min / max over the repeats."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_voxel_raytracer_amd import Context  # noqa: E402
from gpu_voxel_raytracer_amd.host import LIST_UNION  # noqa: E402
from pieces_latency import timed  # noqa: E402
from transform_latency import path_keys  # noqa: E402
from voxelize_latency import DEV  # noqa: E402


def gather16(k):
    """bits 3 i of k, i = 0 .. 15 -> a coordinate"""
    x = k & 0x249249249249
    x = (x | x >> 2) & 0x0C30C30C30C3
    x = (x | x >> 4) & 0x00F00F00F00F
    x = (x | x >> 8) & 0x0000FF0000FF
    x = (x | x >> 16) & 0xFFFF
    return x - 32768


def torch_union(a_pos, a_mrgb, b_pos, b_mrgb):
    keys = torch.cat([path_keys(a_pos.to(torch.int64)), path_keys(b_pos.to(torch.int64))])
    mrgb = torch.cat([a_mrgb, b_mrgb])
    skeys, order = torch.sort(keys, stable=True)
    last = torch.ones(len(skeys), dtype=torch.bool, device=keys.device)
    last[:-1] = skeys[1:] != skeys[:-1]                       # A, then B: the last entry of a position wins
    ukeys, uidx = skeys[last], order[last]
    out_pos = torch.stack([gather16(ukeys >> 2), gather16(ukeys >> 1), gather16(ukeys)], -1).to(torch.int16)
    out_mrgb = mrgb[uidx].clone()
    out_mrgb[:, 0] &= 0x7F
    return out_pos, out_mrgb


def torch_intersect(a_pos, b_pos):
    ka, kb = torch.unique(path_keys(a_pos.to(torch.int64))), torch.unique(path_keys(b_pos.to(torch.int64)))
    both, _ = torch.sort(torch.cat([ka, kb]))
    _, counts = torch.unique_consecutive(both, return_counts=True)
    return int((counts == 2).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--unique", type=int, default=1 << 20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    rng = np.random.default_rng(7)
    side = 256
    cells = rng.choice(side ** 3, args.unique + args.unique // 2, replace=False)
    cells = np.stack([cells // (side * side), cells // side % side, cells % side], -1) - side // 2
    half = args.unique // 2
    lists = []
    for part in (cells[:args.unique], cells[half:]):          # the middle third is in both
        part = part[rng.permutation(len(part))]
        lists.append(torch.as_tensor(np.ascontiguousarray(part, np.int16), device=DEV))
        lists.append(torch.as_tensor(rng.integers(0, 256, (len(part), 4)).astype(np.uint8), device=DEV))
    a_pos, a_mrgb, b_pos, b_mrgb = lists
    with Context(64, 64) as ctx:
        union, (u_pos, u_mrgb) = timed(lambda: ctx.combine_voxels(a_pos, a_mrgb, b_pos, b_mrgb, LIST_UNION), args.repeats)
        count, common = timed(lambda: ctx.count_common(a_pos, b_pos), args.repeats)
        route_union, (r_pos, r_mrgb) = timed(lambda: torch_union(a_pos, a_mrgb, b_pos, b_mrgb), args.repeats)
        route_count, r_common = timed(lambda: torch_intersect(a_pos, b_pos), args.repeats)
    assert torch.equal(u_pos, r_pos) and torch.equal(u_mrgb, r_mrgb), "the two routes disagree"
    assert common == r_common == args.unique - half, (common, r_common)
    result = {"entries": [int(len(a_pos)), int(len(b_pos))], "common": int(common), "union_voxels": int(len(u_pos)), "union": union,
              "count_intersect": count, "torch_union": route_union, "torch_intersect": route_count,
              "union_over_route": union["median_ms"] / route_union["median_ms"], "count_over_route": count["median_ms"] / route_count["median_ms"]}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
