"""Latency of building a scene on the device from a voxel list in device memory (vxrt_set_voxels_device, include/vxrt_device_scene.h)
against the host builder (vxrt_set_voxels).  Writes JSON documents for profiles/device_build/.

Host clock around one synchronous call, median / min / max over repeats (after one warm-up call):
  host      vxrt_set_voxels from numpy arrays (build_octree + flatten_svo on one host thread + the upload)
  device    vxrt_set_voxels_device from torch tensors already on the device
  upload    numpy -> torch upload + vxrt_set_voxels_device (Context.set_voxels_device with numpy arrays)
Cases: menger.vox (160 k), the solid ball at 1.1 M / 8.8 M / 33.5 M voxels in scanline and shuffled order, a sparse depth-15 list past
the host builder's 2^26-node limit, and config 5's 975 M-voxel list (get_voxels of vxrt_set_menger(*CONFIG5)), beside vxrt_set_menger.

    python scripts/device_build_latency.py [--out profiles/device_build/latency.json]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/device_build_latency.py --device-only --calls DIR/calls.json
    python scripts/device_build_latency.py --summarize DIR [--out profiles/device_build/kernel_times.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_voxel_raytracer_amd import Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.scenes import CONFIG5  # noqa: E402

KERNELS = ("bounds_kernel", "bounds_reduce_kernel", "keys_kernel", "radix_hist_kernel", "radix_scan_kernel", "radix_scatter_kernel",
           "flag_count_kernel", "exclusive_scan_kernel", "dedupe_write_kernel", "level_hist_kernel", "level_sum_kernel", "level_write_kernel")


def stats_ms(samples):
    s = np.asarray(samples) * 1e3
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "n": int(len(s))}


def ball(r, shuffled):
    a = np.arange(-r, r, dtype=np.int32)
    g = np.stack(np.meshgrid(a, a, a, indexing="ij"), axis=-1).reshape(-1, 3)
    c = g.astype(np.float64) + 0.5
    pos = g[(c * c).sum(1) < r * r].astype(np.int16)
    if shuffled:
        pos = pos[np.random.default_rng(1).permutation(len(pos))]
    mrgb = np.zeros((len(pos), 4), np.uint8)
    mrgb[:, 1:] = (pos.astype(np.int32) & 0xFF).astype(np.uint8)
    return pos, mrgb


def sparse15():
    rng = np.random.default_rng(11)
    pos = rng.integers(-32768, 32768, (12_000_000, 3)).astype(np.int16)
    return pos, rng.integers(0, 256, (len(pos), 4)).astype(np.uint8)


def config5_list():
    with Context(64, 64) as ctx:
        ctx.set_menger(*CONFIG5)
        return ctx.get_voxels()


CASES = {
    "menger_vox": lambda: scenes.load_scene("menger")[:2],
    "ball_1M_scanline": lambda: ball(64, False), "ball_1M_shuffled": lambda: ball(64, True),
    "ball_9M_scanline": lambda: ball(128, False), "ball_9M_shuffled": lambda: ball(128, True),
    "ball_34M_scanline": lambda: ball(200, False), "ball_34M_shuffled": lambda: ball(200, True),
    "sparse_depth15_12M": sparse15,
    "config5_975M": config5_list,
}
HOST_REFUSES = ("sparse_depth15_12M", "config5_975M")


def scratch_bytes(n):
    """device_build.hip's peak scratch for n voxels: keys 2 x 8 B and leaf words 2 x 4 B per voxel, digit counts, partials, level bins."""
    blocks = (n + 4095) // 4096
    return 24 * n + 256 * blocks * 4 + 256 * 4 + (blocks + 1) * 8 + (17 * blocks + 17) * 8 + 1025 * 8


def timed(fn, repeats):
    fn()
    out = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def run_case(name, repeats, device_only, calls):
    import torch
    pos, mrgb = CASES[name]()
    n = len(pos)
    reps = 3 if n > 100_000_000 else repeats
    res = {"voxels": int(n), "peak_scratch_bytes": int(scratch_bytes(n)), "scratch_bytes_per_voxel": scratch_bytes(n) / max(n, 1)}
    with Context(64, 64) as ctx:
        tp, tm = torch.as_tensor(pos, device="cuda:0"), torch.as_tensor(mrgb, device="cuda:0")
        torch.cuda.synchronize()
        res["device"] = stats_ms(timed(lambda: ctx.set_voxels_device(tp, tm), reps))
        calls.append([name, reps + 1])
        res["octree_nodes"] = int(ctx.stats().octree_nodes)
        del tp, tm
        torch.cuda.empty_cache()
        if device_only:
            return res
        res["upload_and_device"] = stats_ms(timed(lambda: ctx.set_voxels_device(pos, mrgb), reps))
        calls.append([name + " (upload)", reps + 1])
        if name in HOST_REFUSES:
            res["host"] = {"refused": "2^26 octree nodes or more"}
        else:
            res["host"] = stats_ms(timed(lambda: ctx.recreate_octree(pos, mrgb), min(reps, 5)))
            res["speedup_device_vs_host"] = res["host"]["median_ms"] / res["device"]["median_ms"]
        if name == "config5_975M":
            res["set_menger"] = stats_ms(timed(lambda: ctx.set_menger(*CONFIG5), 3))
    return res


def summarize(root):
    """Per-call device time of the build's kernels from one rocprofv3 --kernel-trace run of --device-only (calls.json: the calls in order)."""
    calls = json.load(open(os.path.join(root, "calls.json")))
    found = []   # (start, end, kernel name): the CSV output, or the SQLite database rocprofv3 writes by default
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            found += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    for f in glob.glob(os.path.join(root, "**", "*_results.db"), recursive=True):
        import sqlite3
        with sqlite3.connect(f) as db:
            found += list(db.execute("select start, end, name from kernels"))
    rows = []
    for s, e, k in found:
        name = next((n for n in KERNELS if n + "(" in k or k.endswith(n) or (n in k and "vxrt" in k)), None)
        if name:
            rows.append((int(s), int(e), name))
    rows.sort()
    starts = [i for i, r in enumerate(rows) if r[2] == "bounds_kernel"]   # every call opens with the bounds
    groups = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])]
    out, g = {}, 0
    for case, count in calls:
        mine, g = groups[g:g + count][1:], g + count   # the warm-up call is not counted
        busy = [sum(e - s for s, e, _ in c) / 1e3 for c in mine]
        span = [(c[-1][1] - c[0][0]) / 1e3 for c in mine]
        per = {}
        for c in mine:
            for s, e, k in c:
                per.setdefault(k, []).append((e - s) / 1e3)
        out[case] = {"calls": len(mine), "dispatches_per_call": len(mine[0]) if mine else 0,
                     "kernel_ms_per_call": {"median": float(np.median(busy)) / 1e3, "min": float(np.min(busy)) / 1e3},
                     "first_to_last_dispatch_ms": {"median": float(np.median(span)) / 1e3},
                     "per_kernel_us_sum_per_call": {k: float(np.sum(v)) / max(len(mine), 1) for k, v in per.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), action="append")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--calls")
    ap.add_argument("--summarize")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarize:
        result = summarize(args.summarize)
    else:
        result, calls = {}, []
        for name in args.case or list(CASES):
            result[name] = run_case(name, args.repeats, args.device_only, calls)
            print(name, json.dumps(result[name]), file=sys.stderr, flush=True)
        if args.calls:
            with open(args.calls, "w") as f:
                json.dump(calls, f)
        faster = [r["voxels"] for r in result.values() if "speedup_device_vs_host" in r and r["speedup_device_vs_host"] > 1.0]
        result["crossover_note"] = {"smallest_list_where_device_beats_host": min(faster) if faster else None}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
