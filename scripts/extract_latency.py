"""Latency of reading a scene's voxels back (vxrt_get_voxels, include/vxrt_extract.h), against the host route it replaces
(vxrt_debug_read_scene + a numpy decode of the records).  Writes JSON documents for profiles/extract/.

Host time: a clock around one synchronous vxrt_get_voxels call into preallocated arrays (no numpy allocation inside), warmed (one call
first), median / min / max over repeats.  Cases: the whole menger.vox (count and fetch), the whole config 5 sponge (vxrt_set_menger of
scenes.CONFIG5; count, and fetch when the host has the memory for its 10.5 GB), a 16^3 and a 256^3 box of it (count and fetch).

    python scripts/extract_latency.py [--out profiles/extract/latency.json]      all cases, host clock
    python scripts/extract_latency.py --case c5_box16_fetch --repeats 20        one case (the kernel-trace runs, one process per case:
                                                                                 rocprofv3 --kernel-trace --stats -d DIR/c5_box16 -- python ...)
    python scripts/extract_latency.py --summarize DIR [--out kernel_times.json]  per-call device time of the extract_* kernels (and their scan) of those runs
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_voxel_raytracer_amd import Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.scenes import CONFIG5  # noqa: E402

BOX16 = ((1458, 16, 32), (1474, 32, 48))
BOX256 = ((0, 0, 0), (256, 256, 256))
# name: (scene, box or None, fetch)
CASES = {
    "menger_count": ("menger", None, False), "menger_fetch": ("menger", None, True),
    "c5_count": ("config5", None, False), "c5_fetch": ("config5", None, True),
    "c5_box16_count": ("config5", BOX16, False), "c5_box16_fetch": ("config5", BOX16, True),
    "c5_box256_count": ("config5", BOX256, False), "c5_box256_fetch": ("config5", BOX256, True),
}


def stats_ms(samples):
    s = np.asarray(samples) * 1e3
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "n": int(len(s))}


def host_gib_available():
    try:
        with open("/proc/meminfo") as f:
            for line in f:
                if line.startswith("MemAvailable:"):
                    return int(line.split()[1]) / 2 ** 20
    except OSError:
        pass
    return 0.0


def make_scene(name):
    ctx = Context(256, 256, max_bounces=4)
    if name == "menger":
        pos, mrgb, _ = scenes.load_scene("menger")
        ctx.recreate_octree(pos, mrgb)
    else:
        ctx.set_menger(*CONFIG5)
    return ctx


def call(ctx, box, pos=None, mrgb=None):
    """One vxrt_get_voxels call (count only without arrays) -> its host time in seconds."""
    lo, hi = (None, None) if box is None else (np.asarray(box[0], np.int32), np.asarray(box[1], np.int32))
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)   # noqa: E731
    n = C.c_size_t(0)
    t0 = time.perf_counter()
    rc = ctx._L.vxrt_get_voxels(ctx._h, p(lo), p(hi), p(pos), p(mrgb), C.c_size_t(0 if pos is None else len(pos)), C.byref(n))
    dt = time.perf_counter() - t0
    if rc != 0:
        raise RuntimeError(f"vxrt_get_voxels: {rc} {ctx._L.vxrt_last_error()}")
    return dt, n.value


def run_case(ctx, box, fetch, repeats):
    _, count = call(ctx, box)
    arrays = (np.empty((count, 3), np.int16), np.empty((count, 4), np.uint8)) if fetch else (None, None)
    if fetch:
        arrays[0].fill(0)   # touch the pages once: the copy is timed, not the first-touch faults
        arrays[1].fill(0)
    samples = [call(ctx, box, *arrays)[0] for _ in range(repeats + 1)][1:]
    return {"voxels": int(count), "output_bytes": int(count) * 10 if fetch else 0, **stats_ms(samples)}


def host_route(ctx, depth, box):
    """vxrt_debug_read_scene + the numpy decode (extract_model.decode_records_box; edit_model.decode_records for the whole scene)."""
    import edit_model as M
    import extract_model as X
    t0 = time.perf_counter()
    svo, leaves = ctx.read_scene()
    t1 = time.perf_counter()
    if box is None:
        n = len(M.decode_records(svo, leaves, depth))
    else:
        n = len(X.decode_records_box(svo, leaves, depth, box)[0])
    t2 = time.perf_counter()
    return {"voxels": n, "read_scene_ms": (t1 - t0) * 1e3, "decode_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3,
            "scene_bytes": int(svo.nbytes + leaves.nbytes)}


def summarize(root):
    """Per-call device time of the extract_* kernels of every case run under rocprofv3 --kernel-trace (one directory per case)."""
    out = {}
    for case_dir in sorted(glob.glob(os.path.join(root, "*"))):
        files = glob.glob(os.path.join(case_dir, "**", "*kernel_trace.csv"), recursive=True)
        meta = os.path.join(case_dir + ".json")
        if not files or not os.path.exists(meta):
            continue
        info = json.load(open(meta))
        calls = info["calls"]
        rows = []
        for f in files:
            with open(f) as fh:
                for r in csv.DictReader(fh):
                    if "extract_" in r["Kernel_Name"] or "exclusive_scan" in r["Kernel_Name"]:
                        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
        rows.sort()
        rows = rows[info["skip_dispatches"]:]
        if not rows or len(rows) % calls:
            out[os.path.basename(case_dir)] = {"error": f"{len(rows)} dispatches for {calls} calls"}
            continue
        per = len(rows) // calls
        busy = [sum(e - s for s, e, _ in rows[i * per:(i + 1) * per]) / 1e3 for i in range(calls)]
        span = [(rows[(i + 1) * per - 1][1] - rows[i * per][0]) / 1e3 for i in range(calls)]
        by_kernel = {}
        for s, e, k in rows:
            name = next(n for n in ("extract_count", "exclusive_scan", "extract_expand") if n in k)
            by_kernel.setdefault(name, []).append((e - s) / 1e3)
        out[os.path.basename(case_dir)] = {
            "calls": calls, "dispatches_per_call": per,
            "kernel_us_per_call": {"median": float(np.median(busy)), "min": float(np.min(busy)), "max": float(np.max(busy))},
            "first_to_last_dispatch_us": {"median": float(np.median(span))},
            "per_kernel_us": {k: {"median": float(np.median(v)), "max": float(np.max(v)), "n": len(v)} for k, v in by_kernel.items()},
        }
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--summarize")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarize:
        result = summarize(args.summarize)
    elif args.case:
        scene, box, fetch = CASES[args.case]
        with make_scene(scene) as ctx:
            depth = ctx.stats().octree_depth
            # the dispatches of the case's calls (repeats + the warm-up) follow those of one counting call (3 per node level above the leaf parents, 2 at theirs) when it fetches
            result = {args.case: run_case(ctx, box, fetch, args.repeats), "calls": args.repeats + 1 + (0 if fetch else 1),
                      "skip_dispatches": 3 * depth + 2 if fetch else 0}
    else:
        result = {"cases": {}, "host_route": {}}
        big = host_gib_available() > 48
        for scene in ("menger", "config5"):
            with make_scene(scene) as ctx:
                depth = ctx.stats().octree_depth
                for name, (s, box, fetch) in CASES.items():
                    if s != scene:
                        continue
                    if name == "c5_fetch" and not big:
                        result["cases"][name] = {"skipped": "less than 48 GiB of host memory available"}
                        continue
                    reps = 3 if name == "c5_fetch" else args.repeats
                    result["cases"][name] = run_case(ctx, box, fetch, reps)
                    print(name, json.dumps(result["cases"][name]), file=sys.stderr, flush=True)
                result["host_route"][scene] = host_route(ctx, depth, None if scene == "menger" else BOX16)
                print(scene, "host route", json.dumps(result["host_route"][scene]), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
