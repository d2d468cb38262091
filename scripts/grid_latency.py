"""Latency and peak memory of building a scene from a dense grid in device memory (vxrt_set_voxel_grid, include/vxrt_grid.h) against
the route a user has without it (torch.nonzero + gather + vxrt_set_voxels_device), and of writing a box back as a grid
(vxrt_get_voxel_grid).  Writes JSON documents for profiles/grid/.

Host clock around one synchronous call, median / min / max over repeats (after one warm-up call):
  grid      Context.set_voxel_grid of the grid tensor
  nonzero   torch.nonzero (x slab by x slab: nonzero takes fewer than 2^31 elements) + the palette / word gather + the int16 cast +
            Context.set_voxels_device
  export    Context.get_voxel_grid of the grid's whole box, then torch.cuda.synchronize; GB/s = box bytes / time
Peak device memory: torch.cuda.max_memory_allocated over the call (the grid included, as both routes start from it), plus the builder's
own scratch, which torch does not see: the list builder's from device_build_latency.scratch_bytes, the grid builder's bounded above by
grid_scratch_bytes.
Cases: menger.vox as a grid, balls of diameter 512 and 1024, a 1024^3 grid at 10 % random occupancy, config 5's sponge as a 2048^3
PALETTE8 grid (about 8.6 GB).

    python scripts/grid_latency.py [--out profiles/grid/latency.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/grid_latency.py --grid-only --calls DIR/calls.json
    python scripts/grid_latency.py --summarize DIR [--out profiles/grid/kernel_times.json]
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from gpu_voxel_raytracer_amd import Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.scenes import CONFIG5  # noqa: E402
from device_build_latency import scratch_bytes as list_scratch_bytes, stats_ms, timed  # noqa: E402

DEV = torch.device("cuda", 0)
KERNELS = ("grid_tile_stats_kernel", "grid_tile_reduce_kernel", "grid_tile_code_kernel", "radix_hist_kernel", "radix_scan_kernel",
           "radix_scatter_kernel", "grid_chunk_sum_kernel", "exclusive_scan_kernel", "grid_chunk_offsets_kernel", "grid_emit_kernel",
           "level_hist_kernel", "level_sum_kernel", "flag_count_kernel", "level_write_kernel")
SLAB = 64


def grid_scratch_bytes(cells, m):
    """grid_build.hip's peak scratch, bounded above: per 16^3 tile its stats, codes (2 x 12 B), offset and digit counts; 8 B of key per
    voxel, and at most as much again for the leaf parents' keys; the level scan's partials and bins."""
    tiles = (cells + 4095) // 4096
    blocks = (m + 4095) // 4096
    return tiles * (48 + 24 + 8 + 4) + 16 * m + (blocks + 1) * 8 + (17 * blocks + 17) * 8 + 1025 * 48


def palette_of(seed=3):
    return np.random.default_rng(seed).integers(0, 256, (256, 4)).astype(np.uint8)


def menger_vox():
    pos, mrgb, _ = scenes.load_scene("menger")
    lo = pos.min(axis=0).astype(np.int64)
    dims = tuple(int(v) for v in pos.max(axis=0).astype(np.int64) - lo + 1)
    uniq, inv = np.unique(mrgb.view(np.uint32), return_inverse=True)
    assert len(uniq) <= 255
    pal = np.zeros((256, 4), np.uint8)
    pal[1:len(uniq) + 1] = uniq.view(np.uint8).reshape(-1, 4)
    g = np.zeros(dims, np.uint8)
    p = pos.astype(np.int64) - lo
    g[p[:, 0], p[:, 1], p[:, 2]] = inv.reshape(-1) + 1
    return torch.as_tensor(g, device=DEV), tuple(int(v) for v in lo), pal


def ball(d):
    r = d // 2
    c = torch.arange(-r, r, device=DEV, dtype=torch.int32)
    g = torch.empty((d, d, d), dtype=torch.uint8, device=DEV)
    for x in range(0, d, SLAB):
        xx = c[x:x + SLAB].view(-1, 1, 1)
        inside = xx * xx + c.view(1, -1, 1) ** 2 + c.view(1, 1, -1) ** 2 < r * r
        g[x:x + SLAB] = inside.to(torch.uint8) * (1 + (c.view(1, 1, -1) & 7).to(torch.uint8))
    return g, (-r, -r, -r), palette_of()


def random10(d=1024):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(10)
    g = torch.empty((d, d, d), dtype=torch.uint8, device=DEV)
    for x in range(0, d, SLAB):
        rr = torch.rand((SLAB, d, d), generator=gen, device=DEV)
        g[x:x + SLAB] = torch.where(rr < 0.1, (rr * 2540).to(torch.uint8) + 1, torch.zeros((), dtype=torch.uint8, device=DEV))
    return g, (-d // 2, -d // 2, -d // 2), palette_of()


def config5_grid():
    """vxrt_set_menger(*CONFIG5) written back as a PALETTE8 grid of its 2048^3 box"""
    with Context(64, 64) as ctx:
        ctx.set_menger(*CONFIG5)
        total = ctx.count_voxels()
        origin = next(o for o in ((0, 0, 0), (-1024, -1024, -1024), (-2048, -2048, -2048))
                      if ctx.count_voxels(o, tuple(v + 2048 for v in o)) == total)
        words = set()
        for x in range(0, 2048, SLAB):
            w = ctx.get_voxel_grid((origin[0] + x, origin[1], origin[2]), (SLAB, 2048, 2048))
            words |= set(torch.unique(w).tolist()) - {0}
            del w
        assert len(words) <= 255
        table = torch.tensor(sorted(words), dtype=torch.int64, device=DEV)
        g = torch.empty((2048, 2048, 2048), dtype=torch.uint8, device=DEV)
        for x in range(0, 2048, SLAB):
            w = ctx.get_voxel_grid((origin[0] + x, origin[1], origin[2]), (SLAB, 2048, 2048)).to(torch.int64)
            g[x:x + SLAB] = torch.where(w != 0, torch.searchsorted(table, w) + 1, 0).to(torch.uint8)
            del w
    pal = np.zeros((256, 4), np.uint8)
    for i, w in enumerate(sorted(words)):
        u = w & 0xFFFFFFFF
        pal[i + 1] = ((u >> 24) & 0x7F, (u >> 16) & 0xFF, (u >> 8) & 0xFF, u & 0xFF)
    return g, origin, pal


CASES = {"menger_vox": menger_vox, "ball_512": lambda: ball(512), "ball_1024": lambda: ball(1024), "random10_1024": random10,
         "config5_2048": config5_grid}


def nonzero_route(ctx, g, origin, pal):
    table = torch.as_tensor(pal, device=DEV)
    pos, mrgb = [], []
    for x in range(0, g.shape[0], SLAB):
        slab = g[x:x + SLAB]
        idx = torch.nonzero(slab)
        mrgb.append(table[slab[idx[:, 0], idx[:, 1], idx[:, 2]].long()])
        pos.append((idx + torch.tensor((origin[0] + x, origin[1], origin[2]), device=DEV)).to(torch.int16))
        del idx
    pos, mrgb = torch.cat(pos), torch.cat(mrgb)
    ctx.set_voxels_device(pos, mrgb)
    return len(pos)


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated()


def run_case(name, repeats, grid_only, calls):
    g, origin, pal = CASES[name]()
    torch.cuda.synchronize()
    cells = g.numel()
    big = cells > 2 ** 31
    reps = 3 if big else repeats
    res = {"dims": list(g.shape), "origin": list(origin), "grid_bytes": int(cells)}
    with Context(64, 64) as ctx:
        res["grid"] = stats_ms(timed(lambda: ctx.set_voxel_grid(g, origin, pal), reps))
        calls.append([name, reps + 1])
        m = ctx.count_voxels()
        res["voxels"] = m
        res["octree_nodes"] = int(ctx.stats().octree_nodes)
        if grid_only:
            return res
        res["grid_peak_bytes"] = int(peak(lambda: ctx.set_voxel_grid(g, origin, pal)) + grid_scratch_bytes(cells, m))
        res["grid_scratch_bytes_upper"] = int(grid_scratch_bytes(cells, m))
        res["nonzero"] = stats_ms(timed(lambda: nonzero_route(ctx, g, origin, pal), reps))
        torch.cuda.empty_cache()
        res["nonzero_peak_bytes"] = int(peak(lambda: nonzero_route(ctx, g, origin, pal)) + list_scratch_bytes(m))
        res["speedup_grid_vs_nonzero"] = res["nonzero"]["median_ms"] / res["grid"]["median_ms"]
        shape = tuple(g.shape)
        del g
        torch.cuda.empty_cache()
        out = torch.empty(shape, dtype=torch.int32, device=DEV)

        def export():
            ctx.get_voxel_grid(origin, shape, out=out)
            torch.cuda.synchronize()
        res["export"] = stats_ms(timed(export, reps))
        res["export_GBps"] = cells * 4 / (res["export"]["median_ms"] * 1e-3) / 1e9
    return res


def summarize(root):
    """Per-call device time of set_voxel_grid's kernels from one rocprofv3 --kernel-trace run of --grid-only (calls.json: the calls in
    order; every call opens with grid_tile_stats_kernel)."""
    calls = json.load(open(os.path.join(root, "calls.json")))
    found = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            found += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    for f in glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True):
        import sqlite3
        with sqlite3.connect(f) as db:
            found += list(db.execute("select start, end, name from kernels"))
    rows = []
    for s, e, k in found:
        name = next((n for n in KERNELS if n in k), None)
        if name:
            rows.append((int(s), int(e), name))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if r[2] == "grid_tile_stats_kernel"]
    groups = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])]
    out, g = {}, 0
    for case, count in calls:
        mine, g = groups[g:g + count][1:], g + count
        busy = [sum(e - s for s, e, _ in c) / 1e3 for c in mine]
        per = {}
        for c in mine:
            for s, e, k in c:
                per.setdefault(k, []).append((e - s) / 1e3)
        out[case] = {"calls": len(mine), "kernel_ms_per_call": {"median": float(np.median(busy)) / 1e3, "min": float(np.min(busy)) / 1e3},
                     "per_kernel_us_sum_per_call": {k: float(np.sum(v)) / max(len(mine), 1) for k, v in per.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), action="append")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--grid-only", action="store_true")
    ap.add_argument("--calls")
    ap.add_argument("--summarize")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarize:
        result = summarize(args.summarize)
    else:
        result, calls = {}, []
        for name in args.case or list(CASES):
            result[name] = run_case(name, args.repeats, args.grid_only, calls)
            torch.cuda.empty_cache()
            print(name, json.dumps(result[name]), file=sys.stderr, flush=True)
        if args.calls:
            os.makedirs(os.path.dirname(os.path.abspath(args.calls)), exist_ok=True)
            with open(args.calls, "w") as f:
                json.dump(calls, f)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
