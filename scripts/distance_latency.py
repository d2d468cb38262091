"""Latency of vxrt_distance_voxels_device (include/vxrt_distance.h), read against the routes a host had before it, on the same machine
in the same run.  Prints one JSON document (profiles/distance/).

Lists: the voxels of menger.vox and monu10.vox, and `--unique` distinct random cells of a 256^3 cube, shuffled, already on the device.
Per list DISTANCE_DEPTH, DISTANCE_ERODE, DISTANCE_FIELD and DISTANCE_DILATE at max_d2 1, 16 and 256 (R = 1, 4, 16):
  `distance`  Context.distance_voxels with cap=None: the counting call and the emitting call, positions, bytes and d2
  `count`     the counting call alone
  `morph`     what a host had for the same radius: Context.morph_voxels at connectivity 26 with steps = R (ERODE for DEPTH and ERODE,
              DILATE for FIELD and DILATE).  It grows cubes, not balls: another shape, so a time reference only
  `torch`     a dense grid over the list's bounding box grown by R, the R-bounded minimum over shifted copies axis by axis (exact:
              the squared distance separates), a threshold, nonzero and the sort into path order; positions and d2, no bytes
The script asserts that the call's positions and d2 are the torch route's, in every mode.
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
from gpu_voxel_raytracer_amd.host import (DISTANCE_DEPTH, DISTANCE_DILATE, DISTANCE_ERODE, DISTANCE_FAR, DISTANCE_FIELD, MORPH_DILATE,  # noqa: E402
                                          MORPH_ERODE)
from pieces_latency import timed  # noqa: E402
from transform_latency import path_keys  # noqa: E402
from voxelize_latency import DEV  # noqa: E402

MODES = (("depth", DISTANCE_DEPTH), ("erode", DISTANCE_ERODE), ("field", DISTANCE_FIELD), ("dilate", DISTANCE_DILATE))
BIG = 1 << 14


def radius(max_d2):
    r = 0
    while (r + 1) * (r + 1) <= max_d2:
        r += 1
    return r


def bounded_min(a, axis, r):
    """min over |d| <= r of a shifted by d along the axis + d^2 (a: int32, BIG where there is nothing; its border of r cells is BIG)"""
    out = a.clone()
    n = a.shape[axis]
    for d in range(1, r + 1):
        lo, hi = a.narrow(axis, 0, n - d) + d * d, a.narrow(axis, d, n - d) + d * d
        torch.minimum(out.narrow(axis, d, n - d), lo, out=out.narrow(axis, d, n - d))
        torch.minimum(out.narrow(axis, 0, n - d), hi, out=out.narrow(axis, 0, n - d))
    return out


def torch_route(pos, mode, max_d2):
    """-> (pos int16 [k,3] in path order, d2 int64 [k]); the list must keep R + 1 cells from the ends of the int16 range"""
    r = radius(max_d2)
    p = pos.to(torch.int64)
    lo = p.amin(dim=0) - r - 1
    ext = (p.amax(dim=0) - lo + r + 2).tolist()
    occ = torch.zeros(ext, dtype=torch.bool, device=pos.device)
    q = p - lo
    occ[q[:, 0], q[:, 1], q[:, 2]] = True
    invert = mode in (DISTANCE_DEPTH, DISTANCE_ERODE)
    target = ~occ if invert else occ
    d2 = torch.where(target, 0, BIG).to(torch.int32)
    for axis in range(3):
        d2 = bounded_min(d2, axis, r)
    near = d2 <= max_d2
    keep = occ if mode == DISTANCE_DEPTH else occ & ~near if mode == DISTANCE_ERODE else near & ~occ if mode == DISTANCE_FIELD else near
    cells = torch.nonzero(keep)
    values = torch.where(near, d2, DISTANCE_FAR)[keep].to(torch.int64)
    order = torch.argsort(path_keys(cells + lo))
    return (cells + lo)[order].to(torch.int16), values[order]


def count_only(ctx, pos, mode, max_d2):
    got = C.c_size_t(0)
    ctx._chk(ctx._L.vxrt_distance_voxels_device(ctx._h, C.c_void_p(pos.data_ptr()), None, C.c_size_t(len(pos)), C.c_uint32(mode), C.c_uint32(max_d2),
                                                None, None, None, C.c_size_t(0), C.byref(got)), "vxrt_distance_voxels_device")
    return int(got.value)


def case(ctx, pos, mrgb, repeats):
    out = {"entries": int(len(pos))}
    for max_d2 in (1, 16, 256):
        r = radius(max_d2)
        for name, mode in MODES:
            row = {}
            row["distance"], (d_pos, d_mrgb, d_d2) = timed(lambda: ctx.distance_voxels(pos, mrgb, mode, max_d2), repeats)
            row["count"], _ = timed(lambda: count_only(ctx, pos, mode, max_d2), repeats)
            grow = mode in (DISTANCE_FIELD, DISTANCE_DILATE)
            row["morph"], _ = timed(lambda: ctx.morph_voxels(pos, mrgb, MORPH_DILATE if grow else MORPH_ERODE, 26, r), repeats)
            row["torch"], (t_pos, t_d2) = timed(lambda: torch_route(pos, mode, max_d2), repeats)
            assert torch.equal(d_pos, t_pos), f"{name} at {max_d2}: the two routes disagree on positions"
            assert torch.equal(d_d2.to(torch.int64), t_d2), f"{name} at {max_d2}: the two routes disagree on d2"
            row["voxels"] = int(len(d_pos))
            row["distance_over_torch"] = row["distance"]["median_ms"] / row["torch"]["median_ms"]
            row["distance_over_morph"] = row["distance"]["median_ms"] / row["morph"]["median_ms"]
            out[f"{name}_{max_d2}"] = row
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
