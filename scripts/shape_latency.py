"""Latency of vxrt_shape_voxels_device (include/vxrt_shape.h), read against the route a host had before it and against A/B builds of
the feature itself, on the same machine in the same run.  Prints one JSON document (profiles/shapes/).

Rows: balls of radius 16, 64 and 256 cells about a point off the tile grid, and a slanted capsule of radius 8 and length 1000, each
in the box its host helper gives.
  `count`          the counting call alone (out_pos == out_mrgb == NULL)
  `call`           one writing call with room for exactly the count (it counts, then writes)
  `torch_producer` what a host did: a dense float32 mask over the same box in torch, nonzero, the offset and the int16 cast
  `call_plus_edit` / `torch_plus_edit`   either list through vxrt_edit_voxels_device into a small scene (menger level 2): today's list
                   arrives unsorted, the call's in path order; the edit's front keys and sorts both.  Not at radius 256 (70 M voxels).
The script asserts that the call's count equals the model-free count of the exact rule evaluated with torch in int64.
  --ab tag=path    the same rows (count, call) measured in a child process per A/B library (scripts/ab_build.sh), asserted to give
                   the same bytes as this process's library by a hash of the result
Host clock around the synchronous call, after one warm-up, median / min / max over the repeats."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_voxel_raytracer_amd import Context  # noqa: E402
from gpu_voxel_raytracer_amd.host import ball_shape, capsule_shape  # noqa: E402
from pieces_latency import timed  # noqa: E402
from voxelize_latency import DEV  # noqa: E402

MRGB = (3, 200, 40, 10)
CENTRE = (3.5, -7.25, 11.0)
CAPSULE_A = np.array((-300.0, -220.5, -330.25))
CAPSULE_B = CAPSULE_A + 1000.0 * np.array((0.6, 0.45, 0.66)) / np.linalg.norm((0.6, 0.45, 0.66))      # 1000 cells long, slanted on every axis
EDIT_LIMIT = 5_000_000


def cases():
    out = {f"ball r={r}": ball_shape(CENTRE, r) for r in (16, 64, 256)}
    out["capsule r=8 l=1000"] = capsule_shape(CAPSULE_A.tolist(), CAPSULE_B.tolist(), 8)
    return out


def count_only(ctx, shape, pull, lo, hi):
    got = C.c_size_t(0)
    blo, bhi = (C.c_int32 * 3)(*lo), (C.c_int32 * 3)(*hi)
    with ctx._ordered():
        ctx._chk(ctx._L.vxrt_shape_voxels_device(ctx._h, C.byref(shape), C.byref(pull), blo, bhi, None, None, None, C.c_size_t(0), C.byref(got)),
                 "vxrt_shape_voxels_device")
    return int(got.value)


def exact_count(shape, pull, lo, hi):
    """the rule in torch int64, slab by slab along x: ball and capsule only"""
    total = 0
    m, t = [[int(v) for v in row] for row in pull.m], [int(v) for v in pull.t]
    rr, h2 = (2 * int(shape.r)) ** 2, 2 * int(shape.h[2])
    ys = 2 * torch.arange(lo[1], hi[1], dtype=torch.int64, device=DEV) + 1
    zs = 2 * torch.arange(lo[2], hi[2], dtype=torch.int64, device=DEV) + 1
    for x0 in range(lo[0], hi[0], 32):
        xs = 2 * torch.arange(x0, min(x0 + 32, hi[0]), dtype=torch.int64, device=DEV) + 1
        p = [m[i][0] * xs[:, None, None] + m[i][1] * ys[None, :, None] + m[i][2] * zs[None, None, :] + 2 * t[i] for i in range(3)]
        near = (p[0].abs() < 2 ** 31) & (p[1].abs() < 2 ** 31) & (p[2].abs() < 2 ** 31)
        e = p[2] - p[2].clamp(-h2, h2)
        d2 = torch.where(near, p[0] * p[0] + p[1] * p[1] + e * e, torch.full_like(e, rr + 1))
        total += int((d2 <= rr).sum())
    return total


def torch_ball(centre, radius, lo, hi):
    ax = [torch.arange(lo[i], hi[i], dtype=torch.float32, device=DEV) + (0.5 - centre[i]) for i in range(3)]
    mask = ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2 <= radius * radius
    return (mask.nonzero() + torch.tensor(lo, device=DEV)).to(torch.int16)


def torch_capsule(a, b, radius, lo, hi):
    a, b = torch.tensor(a, dtype=torch.float32, device=DEV), torch.tensor(b, dtype=torch.float32, device=DEV)
    u = (b - a) / torch.linalg.norm(b - a)
    length = float(torch.linalg.norm(b - a))
    ax = [torch.arange(lo[i], hi[i], dtype=torch.float32, device=DEV) + 0.5 - a[i] for i in range(3)]
    along = (ax[0] * u[0])[:, None, None] + (ax[1] * u[1])[None, :, None] + (ax[2] * u[2])[None, None, :]
    along = along.clamp_(0.0, length)
    d2 = (ax[0][:, None, None] - along * u[0]) ** 2
    d2 += (ax[1][None, :, None] - along * u[1]) ** 2
    d2 += (ax[2][None, None, :] - along * u[2]) ** 2
    return ((d2 <= radius * radius).nonzero() + torch.tensor(lo, device=DEV)).to(torch.int16)


def digest(pos, mrgb):
    return hashlib.sha256(pos.cpu().numpy().tobytes() + mrgb.cpu().numpy().tobytes()).hexdigest()[:16]


def measure(repeats, with_torch):
    result = {}
    with Context(64, 64) as ctx, Context(64, 64) as scene:
        scene.set_menger(2)
        for name, (shape, pull, lo, hi) in cases().items():
            count, k = timed(lambda: count_only(ctx, shape, pull, lo, hi), repeats)
            call, (pos, mrgb) = timed(lambda: ctx.shape_voxels(shape, pull, lo, hi, MRGB, cap=k), repeats)
            row = {"box": [list(lo), list(hi)], "cells": int(np.prod([b - a for a, b in zip(lo, hi)])), "voxels": k, "count": count, "call": call,
                   "sha": digest(pos, mrgb)}
            if with_torch:
                assert k == exact_count(shape, pull, lo, hi), name
                if name.startswith("ball"):
                    radius = int(shape.r) / 65536.0
                    producer, t_pos = timed(lambda: torch_ball(CENTRE, radius, lo, hi), repeats)
                else:
                    producer, t_pos = timed(lambda: torch_capsule(CAPSULE_A.tolist(), CAPSULE_B.tolist(), 8.0, lo, hi), repeats)
                row["torch_producer"] = producer
                row["torch_voxels"] = int(len(t_pos))            # float32: may differ from the exact rule's count by a few cells
                row["call_over_torch_producer"] = call["median_ms"] / producer["median_ms"]
                if k <= EDIT_LIMIT:
                    t_mrgb = torch.tensor(MRGB, dtype=torch.uint8, device=DEV).repeat(len(t_pos), 1)
                    row["edit_of_call_list"], _ = timed(lambda: scene.edit_voxels_device(pos, mrgb, grow=True), repeats)
                    row["edit_of_torch_list"], _ = timed(lambda: scene.edit_voxels_device(t_pos, t_mrgb, grow=True), repeats)
                    row["call_plus_edit_ms"] = call["median_ms"] + row["edit_of_call_list"]["median_ms"]
                    row["torch_plus_edit_ms"] = producer["median_ms"] + row["edit_of_torch_list"]["median_ms"]
                del t_pos
            del pos, mrgb
            torch.cuda.empty_cache()
            result[name] = row
            print(json.dumps({name: row}), file=sys.stderr, flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    ap.add_argument("--ab", action="append", default=[], help="tag=path of an A/B library to measure in a child process")
    ap.add_argument("--child", action="store_true", help="measure count and call only, print the JSON")
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.repeats, False)))
        return
    result = {"product": measure(args.repeats, True), "ab": {}}
    for spec in args.ab:
        tag, path = spec.split("=", 1)
        env = dict(os.environ, VXRT_LIB=os.path.abspath(path))
        run = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--repeats", str(args.repeats)], env=env, capture_output=True, text=True,
                             timeout=900)
        assert run.returncode == 0, run.stderr[-2000:]
        rows = json.loads(run.stdout.strip().splitlines()[-1])
        for name, row in rows.items():
            assert row["sha"] == result["product"][name]["sha"] and row["voxels"] == result["product"][name]["voxels"], (tag, name)
            row["call_over_product"] = row["call"]["median_ms"] / result["product"][name]["call"]["median_ms"]
            row["count_over_product"] = row["count"]["median_ms"] / result["product"][name]["count"]["median_ms"]
        result["ab"][tag] = rows
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
