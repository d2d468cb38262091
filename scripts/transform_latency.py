"""Latency of vxrt_transform_voxels_device (include/vxrt_transform.h), read against the route a host had before it, on the same machine
in the same run.  Prints one JSON document (profiles/transform/).

Rows: menger.vox's and monu10.vox's own lists (tests/golden/scenes/) and one detached piece (the sponge's, as the tests break it
off), each already on the device and rotated about its centre of mass by a general rotation into its rigid_box.
  `transform`    Context.transform_voxels: the counting call and the emitting call
  `count`        the counting call alone
  `torch_route`  the same bytes with torch: the box's cells by arange, the pull in int64, path keys, searchsorted on the sorted unique
                 keys of the list, nonzero, a sort by key
The script asserts that both routes give the same bytes.
  `pull_kernel`  the pull kernel's own time at a box of 2^24 cells: the counting call into a 256^3 box under a map that magnifies the
                 list's bounding box to fill it (so no block leaves at the bounding-box test and every cell searches), less the
                 counting call into a one-cell box (the key pass, the sort and the dedupe of the list, which both pay)
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
from gpu_voxel_raytracer_amd import Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.host import Affine, rigid_box, rigid_pull  # noqa: E402
from pieces_latency import timed  # noqa: E402
from voxelize_latency import DEV  # noqa: E402

MENGER_MRGB = (0, 0xB0, 0xD0, 0x60)
SIDE = 256          # the kernel row's box: SIDE^3 = 2^24 cells


def rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1 - np.cos(angle)) * (k @ k)


ROTATION = rotation((1, 2, 3), 0.7)


def spread16(v):
    x = v & 0xFFFF
    x = (x | x << 16) & 0x0000FF0000FF
    x = (x | x << 8) & 0x00F00F00F00F
    x = (x | x << 4) & 0x0C30C30C30C3
    x = (x | x << 2) & 0x249249249249
    return x


def path_keys(p):
    """int64 [n,3] cells of the int16 range -> their path keys at depth 15"""
    u = p + 32768
    return spread16(u[:, 0]) << 2 | spread16(u[:, 1]) << 1 | spread16(u[:, 2])


def torch_route(pos, mrgb, pull, box_min, box_max):
    """the route a host had: everything in torch, the rule's integers in int64"""
    skeys, order = torch.sort(path_keys(pos.to(torch.int64)), stable=True)
    last = torch.ones(len(skeys), dtype=torch.bool, device=pos.device)
    last[:-1] = skeys[1:] != skeys[:-1]                       # the last entry of a position wins
    ukeys, uidx = skeys[last], order[last]
    axes = [torch.arange(int(box_min[ax]), int(box_max[ax]), dtype=torch.int64, device=pos.device) for ax in range(3)]
    d = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    c = 2 * d + 1
    s = torch.stack([(int(pull.m[i][0]) * c[:, 0] + int(pull.m[i][1]) * c[:, 1] + int(pull.m[i][2]) * c[:, 2] + 2 * int(pull.t[i])) >> 17 for i in range(3)], -1)
    ok = ((s >= -32768) & (s <= 32767)).all(dim=1)
    qkeys = path_keys(s.clamp(-32768, 32767))
    at = torch.searchsorted(ukeys, qkeys).clamp(max=len(ukeys) - 1)
    found = (ok & (ukeys[at] == qkeys)).nonzero().reshape(-1)
    _, by_path = torch.sort(path_keys(d[found]))
    found = found[by_path]
    out_mrgb = mrgb[uidx[at[found]]].clone()
    out_mrgb[:, 0] &= 0x7F
    return d[found].to(torch.int16), out_mrgb


def magnify(lo, hi):
    """-> (pull, box_min, box_max): the 256^3 box whose cells pull into the list's bounding box lo .. hi (inclusive), and only there"""
    a = Affine()
    for ax in range(3):
        step = int(np.floor((int(hi[ax]) + 1 - int(lo[ax])) * 65536 / SIDE))          # Q16 source cells per destination cell, rounded down
        a.m[ax][ax] = step
        a.t[ax] = int(lo[ax]) * 65536 + (SIDE // 2) * step
    return a, (-SIDE // 2,) * 3, (SIDE // 2,) * 3


def case(ctx, pos, mrgb, centre, repeats):
    d_pos = torch.as_tensor(np.ascontiguousarray(pos, np.int16), device=DEV)
    d_mrgb = torch.as_tensor(np.ascontiguousarray(mrgb, np.uint8), device=DEV)
    lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
    pull = rigid_pull(ROTATION, centre)
    box = rigid_box(lo, hi, ROTATION, centre)
    cells = int(np.prod([b - a for a, b in zip(*box)]))
    transform, (t_pos, t_mrgb) = timed(lambda: ctx.transform_voxels(d_pos, d_mrgb, pull, *box), repeats)
    count, _ = timed(lambda: count_only(ctx, d_pos, d_mrgb, pull, box), repeats)
    route, (r_pos, r_mrgb) = timed(lambda: torch_route(d_pos, d_mrgb, pull, *box), repeats)
    assert torch.equal(t_pos, r_pos) and torch.equal(t_mrgb, r_mrgb), "the two routes disagree"
    big_pull, big_lo, big_hi = magnify(lo, hi)
    big, big_count = timed(lambda: count_only(ctx, d_pos, d_mrgb, big_pull, (big_lo, big_hi)), repeats)
    front, _ = timed(lambda: count_only(ctx, d_pos, d_mrgb, big_pull, ((0, 0, 0), (1, 1, 1))), repeats)
    return {"entries": int(len(pos)), "box": [list(box[0]), list(box[1])], "cells": cells, "voxels": int(len(t_pos)),
            "transform": transform, "count": count, "torch_route": route, "transform_over_route": transform["median_ms"] / route["median_ms"],
            "pull_kernel": {"cells": SIDE ** 3, "voxels": int(big_count), "count_call": big, "one_cell_call": front,
                            "median_ms": big["median_ms"] - front["median_ms"]}}


def count_only(ctx, d_pos, d_mrgb, pull, box):
    import ctypes as C
    got = C.c_size_t(0)
    lo, hi = (C.c_int32 * 3)(*[int(v) for v in box[0]]), (C.c_int32 * 3)(*[int(v) for v in box[1]])
    with ctx._ordered():
        ctx._chk(ctx._L.vxrt_transform_voxels_device(ctx._h, C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_mrgb.data_ptr()), C.c_size_t(len(d_pos)),
                                                      C.byref(pull), lo, hi, None, None, C.c_size_t(0), C.byref(got)), "vxrt_transform_voxels_device")
    return int(got.value)


def detached_piece(ctx):
    """the sponge's upper part, cut loose one layer above its base -> (pos, mrgb, centre of mass)"""
    ctx.set_menger(3, 0, MENGER_MRGB)
    pos, _ = ctx.get_voxels()
    lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
    ctx.clear_voxels_device(torch.as_tensor(pos[pos[:, 1] == lo[1] + 8], device=DEV))
    p_pos, p_mrgb, _, table = ctx.drop_detached_pieces(tuple(lo.tolist()), (int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))
    centre = (table["sum"].cpu().numpy()[0] / int(table["voxels"][0]) + 0.5).tolist()
    return p_pos.cpu().numpy(), p_mrgb.cpu().numpy(), centre


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    result = {}
    with Context(64, 64) as ctx:
        for name in ("menger", "monu10"):
            pos, mrgb, _ = scenes.load_scene(name)
            pos, mrgb = np.ascontiguousarray(pos, np.int16), np.ascontiguousarray(mrgb, np.uint8)
            centre = (pos.astype(np.float64).mean(axis=0) + 0.5).tolist()
            result[name + ".vox"] = case(ctx, pos, mrgb, centre, args.repeats)
            print(json.dumps({name: result[name + ".vox"]}), file=sys.stderr, flush=True)
        result["detached piece"] = case(ctx, *detached_piece(ctx), args.repeats)
        print(json.dumps({"piece": result["detached piece"]}), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
