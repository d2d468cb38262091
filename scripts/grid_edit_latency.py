"""Latency of writing a dense grid into a box of a loaded scene (vxrt_edit_voxel_grid) against the two routes a host had before it:
the torch diff -> host lists -> two vxrt_edit_voxels calls ("host"), and a rebuild of the whole scene from a grid with
vxrt_set_voxel_grid ("rebuild").  Prints one JSON document (profiles/grid_edit/).

Scenes: menger.vox and BASELINE config 5's sponge (vxrt_set_menger(*CONFIG5)).  Cases: a 64^3 box under REPLACE with 0 changed
cells, 1, 1 %, 10 % and 100 % of its cells changed; sphere brushes of radius 8 and 32 under SET and CLEAR.  Every timed call starts
from the same scene: the box is put back (REPLACE of the saved box, untimed) after each.  Host clock around the synchronous call,
after one warm-up, median / min / max over the repeats; the grid is on the device before the clock starts.  The two routes are
checked to leave identical bytes.
  --device-only   only the grid-edit calls (the kernel-trace run):
                  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/grid_edit_latency.py --device-only --calls DIR/calls.json
  --summarize DIR per-call kernel time of those calls (every call opens with grid_edit_diff_kernel)"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_voxel_raytracer_amd import Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.scenes import CONFIG5  # noqa: E402

DEV = torch.device("cuda", 0)
KERNELS = ("grid_edit_outside_kernel", "grid_edit_diff_kernel", "grid_tile_reduce_kernel", "grid_tile_code_kernel", "radix_hist_kernel",
           "radix_scan_kernel", "radix_scatter_kernel", "grid_chunk_sum_kernel", "exclusive_scan_kernel", "grid_chunk_offsets_kernel",
           "grid_edit_emit_kernel", "cut_count_kernel", "cut_offsets_kernel", "cut_write_kernel", "edit_kernel")


def stats_ms(samples):
    s = np.asarray(samples) * 1e3
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "n": int(len(s))}


def sync_timed(fn):
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(DEV)
    return time.perf_counter() - t0, out


def host_route(ctx, cells, origin, mode):
    """the route without vxrt_edit_voxel_grid: diff in torch, nonzero, both lists to the host, clear_voxels then edit_voxels"""
    s = ctx.get_voxel_grid(origin, cells.shape)
    occ = cells < 0                                                   # bit 31 set
    if mode == "replace":
        clear, sets = (s != 0) & ~occ, occ & (s != cells)
    elif mode == "set":
        clear, sets = torch.zeros_like(occ), occ & (s != cells)
    else:
        clear, sets = (s != 0) & occ, torch.zeros_like(occ)
    o = torch.tensor(origin, device=DEV, dtype=torch.int64)
    cpos = (torch.nonzero(clear) + o).to(torch.int16).cpu().numpy()
    sidx = torch.nonzero(sets)
    spos = (sidx + o).to(torch.int16).cpu().numpy()
    w = cells[sets].cpu().numpy().view(np.uint32)
    mrgb = np.stack([(w >> 24) & 0x7F, (w >> 16) & 0xFF, (w >> 8) & 0xFF, w & 0xFF], 1).astype(np.uint8)
    if len(cpos):
        ctx.clear_voxels(cpos)
    if len(spos):
        ctx.edit_voxels(spos, mrgb)
    return len(spos), len(cpos)


def changed_box(box, fraction, gen):
    """the box with `fraction` of its cells changed: empty cells filled, occupied ones cleared or recoloured"""
    n = box.numel()
    k = int(round(fraction * n)) if fraction >= 0 else 1
    flat = box.reshape(-1).clone()
    pick = torch.randperm(n, generator=gen, device=DEV)[:k]
    colour = torch.randint(0, 1 << 31, (k,), generator=gen, device=DEV, dtype=torch.int64) | (1 << 31)
    colour = (colour - (1 << 32)).to(torch.int32)
    cur = flat[pick]
    drop = torch.rand(k, generator=gen, device=DEV) < 0.5
    flat[pick] = torch.where(cur < 0, torch.where(drop, torch.zeros_like(cur), colour ^ 1), colour)
    return flat.reshape(box.shape)


def sphere(r, gen):
    d = 2 * r + 1
    ax = torch.arange(d, device=DEV) - r
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    colour = int(torch.randint(0, 1 << 31, (1,), generator=gen, device=DEV)) | (1 << 31)
    return torch.where(x * x + y * y + z * z <= r * r, torch.tensor(colour - (1 << 32), device=DEV, dtype=torch.int32),
                       torch.zeros((), device=DEV, dtype=torch.int32))


def cases(gen):
    for name, frac in (("replace 0", 0.0), ("replace 1 cell", -1), ("replace 1%", 0.01), ("replace 10%", 0.1), ("replace 100%", 1.0)):
        yield name, "replace", 64, (lambda box, f=frac: changed_box(box, f, gen))
    for r in (8, 32):
        for mode in ("set", "clear"):
            yield f"sphere r{r} {mode}", mode, 2 * r + 1, (lambda box, r=r: sphere(r, gen))


def load(ctx, name):
    if name == "config5":
        ctx.set_menger(*CONFIG5)
    else:
        pos, mrgb, size = scenes.load_scene(name)
        ctx.recreate_octree(pos, mrgb)
    h = 1 << ctx.stats().octree_depth
    # the 64^3 box with the most voxels among a few placements across the scene
    places = [(v, v, v) for v in (-h // 2, -h // 4, 0, 4, h // 8, h // 4, h // 3, h // 2)]
    return max(places, key=lambda o: int((ctx.get_voxel_grid(o, (64, 64, 64)) != 0).sum()))


def run_scene(name, repeats, device_only, calls):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    out = {}
    with Context(64, 64) as a, Context(64, 64) as b:
        box0 = load(a, name)
        if not device_only:
            load(b, name)
        depth = a.stats().octree_depth
        for case, mode, side, make in cases(gen):
            origin = box0 if side == 64 else tuple(v + 32 - side // 2 for v in box0)
            saved = a.get_voxel_grid(origin, (side,) * 3).clone()
            cells = make(saved)
            row = {"mode": mode, "box": side, "cells_changed": None}
            grid, host, counts = [], [], None
            for r in range(repeats + 1):
                dt, counts = sync_timed(lambda: a.edit_voxel_grid(cells, origin, mode=mode))
                a.edit_voxel_grid(saved, origin)                  # put the box back (untimed)
                calls.append([f"{name} {case}", "timed" if r else "warm"])
                calls.append([f"{name} {case}", "restore"])
                if r:
                    grid.append(dt)
                if not device_only:
                    dt, hc = sync_timed(lambda: host_route(b, cells, origin, mode))
                    assert hc == counts, (case, hc, counts)
                    b.edit_voxel_grid(saved, origin)
                    if r:
                        host.append(dt)
            row["cells_changed"] = {"set": counts[0], "cleared": counts[1]}
            row["grid_edit"] = stats_ms(grid)
            if not device_only:
                row["host_route"] = stats_ms(host)
                # both contexts went through the same edits, each by its own route: one more of each, then the bytes
                a.edit_voxel_grid(cells, origin, mode=mode)
                host_route(b, cells, origin, mode)
                sa, la = a.read_scene()
                sb, lb = b.read_scene()
                row["identical_bytes"] = bool(np.array_equal(sa, sb) and np.array_equal(la, lb))
                a.edit_voxel_grid(saved, origin)
                b.edit_voxel_grid(saved, origin)
            out[case] = row
            print(json.dumps({name: {case: row}}), file=sys.stderr, flush=True)
        if not device_only and name != "config5":
            # the rebuild route: the whole scene's root cube as a grid, vxrt_set_voxel_grid
            h = 1 << depth
            whole = a.get_voxel_grid((-h, -h, -h), (2 * h,) * 3)
            with Context(64, 64) as c:
                samples = [sync_timed(lambda: c.set_voxel_grid(whole, (-h, -h, -h)))[0] for _ in range(4)][1:]
            out["rebuild (set_voxel_grid of the root cube)"] = stats_ms(samples)
    return out


def summarize(root):
    calls = json.load(open(os.path.join(root, "calls.json")))
    found = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            found += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows = sorted((s, e, next(n for n in KERNELS if n in k)) for s, e, k in found if any(n in k for n in KERNELS))
    starts = [i for i, r in enumerate(rows) if r[2] == "grid_edit_diff_kernel"]
    groups = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])]
    assert len(groups) == len(calls), (len(groups), len(calls))
    out = {}
    for (case, kind), g in zip(calls, groups):
        if kind != "timed":
            continue
        c = out.setdefault(case, {"busy_us": [], "per_kernel_us": {}})
        c["busy_us"].append(sum(e - s for s, e, _ in g) / 1e3)
        for s, e, k in g:
            c["per_kernel_us"].setdefault(k, []).append((e - s) / 1e3)
    return {case: {"calls": len(c["busy_us"]), "kernel_ms_per_call": {"median": float(np.median(c["busy_us"])) / 1e3,
                                                                       "min": float(np.min(c["busy_us"])) / 1e3},
                   "per_kernel_us_per_call": {k: float(np.sum(v)) / len(c["busy_us"]) for k, v in c["per_kernel_us"].items()}}
            for case, c in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", help="write the list of grid-edit calls here (for --summarize)")
    ap.add_argument("--summarize")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarize:
        result = summarize(args.summarize)
    else:
        calls = []
        result = {name: run_scene(name, args.repeats, args.device_only, calls) for name in ("menger", "config5")}
        if args.calls:   # under rocprofv3 -d DIR, DIR is only made when the program ends
            os.makedirs(os.path.dirname(os.path.abspath(args.calls)), exist_ok=True)
            json.dump(calls, open(args.calls, "w"))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
