"""Latency of voxelising a triangle mesh on the device (vxrt_voxelize_mesh_device, include/vxrt_voxelize.h).  There is no earlier
route in the project to compare against, so this records what is measured.  Prints one JSON document (profiles/voxelize/).

Meshes: an icosphere at three sizes (4, 6 and 7 subdivisions: 5 120, 81 920 and 327 680 triangles, radius 50, 200 and 800 voxels) and
"mixed": the middle sphere plus four triangles some 3 000 voxels across cutting through it, so that a few triangles own most of the
work items.  Per mesh, host clock around the synchronous call with the mesh already on the device, after one warm-up, median / min /
max over the repeats: "count" (pos == mrgb == NULL), "fetch" (one run into arrays with room to spare) and "count_then_fetch"
(Context.voxelize_mesh without cap: both, plus the allocation of the result).
  --device-only   only the fetch calls (the kernel-trace run):
                  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/voxelize_latency.py --device-only --calls DIR/calls.json
  --summarize DIR per-call kernel time of those calls, split into the front (the vox_* kernels and their scans), sort_unique_list
                  (the radix sort and the dedupe) and the decode"""
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
from gpu_voxel_raytracer_amd import Context  # noqa: E402

DEV = torch.device("cuda", 0)
FRONT = ("vox_setup_kernel", "vox_reduce_kernel", "vox_offsets_kernel", "vox_walk_kernel")
SORT = ("radix_hist_kernel", "radix_scan_kernel", "radix_scatter_kernel", "flag_count_kernel", "dedupe_write_kernel")
KERNELS = FRONT + SORT + ("exclusive_scan_kernel", "vox_decode_kernel")


def icosphere(subdivisions, radius, centre=(0.5, 0.5, 0.5)):
    phi = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, phi, 0), (1, phi, 0), (-1, -phi, 0), (1, -phi, 0), (0, -1, phi), (0, 1, phi), (0, -1, -phi), (0, 1, -phi),
                  (phi, 0, -1), (phi, 0, 1), (-phi, 0, -1), (-phi, 0, 1)], np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    t = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)], np.int64)
    for _ in range(subdivisions):
        edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1)
        uniq, inverse = np.unique(edges, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inverse.reshape(3, -1)          # the midpoint's index of each triangle's edges ab, bc, ca
        v = np.concatenate([v, mid])
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        t = np.concatenate([np.stack(x, axis=1) for x in ((a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2]))])
    return (v * radius + np.array(centre)).astype(np.float32), t.astype(np.uint32)


def meshes():
    out = {}
    for sub, radius in ((4, 50.0), (6, 200.0), (7, 800.0)):
        out[f"icosphere {sub}"] = icosphere(sub, radius)
    v, t = out["icosphere 6"]
    big = np.array([(-1500.3, -1400.1, 20.2), (1490.7, -1300.9, -170.4), (-200.2, 1510.6, 220.8),
                    (30.1, -1450.2, -1500.5), (-60.7, 1480.3, -1390.9), (90.4, 100.6, 1520.2)], np.float32)
    bt = np.array([(0, 1, 2), (3, 4, 5), (0, 4, 5), (1, 2, 3)], np.uint32) + len(v)
    keep = np.random.default_rng(1).permutation(len(t) + 4)     # the large triangles somewhere among the small ones
    out["mixed"] = (np.concatenate([v, big]), np.concatenate([t, bt])[keep])
    return out


def stats_ms(samples):
    s = np.asarray(samples) * 1e3
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "n": int(len(s))}


def sync_timed(fn):
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(DEV)
    return time.perf_counter() - t0, out


def run(repeats, device_only, calls):
    import ctypes as C
    out = {}
    with Context(64, 64) as ctx:
        for name, (v, t) in meshes().items():
            k = np.arange(len(t))
            m = np.stack([k % 128, k % 256, (k // 7) % 256, (k // 256) % 256], axis=1).astype(np.uint8)
            dv, dt, dm = torch.as_tensor(v, device=DEV), torch.as_tensor(t.view(np.int32), device=DEV), torch.as_tensor(m, device=DEV)
            n = len(ctx.voxelize_mesh(dv, dt, dm)[0])
            calls.append([name, "warm"])
            got = C.c_size_t(0)
            args = (ctx._h, C.c_void_p(dv.data_ptr()), C.c_size_t(len(dv)), C.c_void_p(dt.data_ptr()), C.c_void_p(dm.data_ptr()), C.c_size_t(len(dt)))
            pos, mrgb = torch.empty((n + 16, 3), dtype=torch.int16, device=DEV), torch.empty((n + 16, 4), dtype=torch.uint8, device=DEV)

            def count():
                assert ctx._L.vxrt_voxelize_mesh_device(*args, None, None, C.c_size_t(0), C.byref(got)) == 0 and got.value == n

            def fetch():
                assert ctx._L.vxrt_voxelize_mesh_device(*args, C.c_void_p(pos.data_ptr()), C.c_void_p(mrgb.data_ptr()), C.c_size_t(n + 16),
                                                        C.byref(got)) == 0 and got.value == n
            samples = {"count": [], "fetch": [], "count_then_fetch": []}
            for r in range(repeats + 1):
                todo = (("fetch", fetch),) if device_only else (("count", count), ("fetch", fetch), ("count_then_fetch", lambda: ctx.voxelize_mesh(dv, dt, dm)))
                for what, fn in todo:
                    dt_s, _ = sync_timed(fn)
                    if r:
                        samples[what].append(dt_s)
                calls.append([name, "timed" if r else "warm"])
            out[name] = {"triangles": int(len(t)), "voxels": int(n), **{w: stats_ms(s) for w, s in samples.items() if s}}
            print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    return out


def summarize(root):
    calls = json.load(open(os.path.join(root, "calls.json")))
    found = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            found += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows = sorted((s, e, next(n for n in KERNELS if n in k)) for s, e, k in found if any(n in k for n in KERNELS))
    starts = [i for i, r in enumerate(rows) if r[2] == "vox_setup_kernel"]
    groups = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])]
    groups = [g for g in groups if any(r[2] == "vox_decode_kernel" for r in g)]       # the fetch calls (the first call per mesh counts first)
    assert len(groups) == len(calls), (len(groups), len(calls))
    out = {}
    for (case, kind), g in zip(calls, groups):
        if kind != "timed":
            continue
        c = out.setdefault(case, {"front": [], "sort_unique_list": [], "decode": [], "per_kernel_us": {}})
        part = {"front": 0, "sort_unique_list": 0, "decode": 0}
        for i, (s, e, k) in enumerate(g):
            where = ("front" if k in FRONT else "sort_unique_list" if k in SORT else "decode" if k == "vox_decode_kernel" else
                     "sort_unique_list" if g[i - 1][2] == "flag_count_kernel" else "front")
            part[where] += e - s
            c["per_kernel_us"].setdefault(k, []).append((e - s) / 1e3)
        for w, ns in part.items():
            c[w].append(ns / 1e6)
    return {case: {"calls": len(c["front"]),
                   **{w: {"median_ms": float(np.median(c[w])), "min_ms": float(np.min(c[w])), "max_ms": float(np.max(c[w]))}
                      for w in ("front", "sort_unique_list", "decode")},
                   "per_kernel_us_per_call": {k: float(np.sum(v)) / len(c["front"]) for k, v in c["per_kernel_us"].items()}}
            for case, c in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", help="write the list of fetch calls here (for --summarize)")
    ap.add_argument("--summarize")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarize:
        result = summarize(args.summarize)
    else:
        calls = []
        result = run(args.repeats, args.device_only, calls)
        if args.calls:   # under rocprofv3 -d DIR, DIR is only made when the program ends
            os.makedirs(os.path.dirname(os.path.abspath(args.calls)), exist_ok=True)
            json.dump(calls, open(args.calls, "w"))
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
