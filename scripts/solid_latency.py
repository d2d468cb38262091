"""Latency of voxelising a closed mesh as a solid on the device (vxrt_voxelize_solid_device, include/vxrt_solid.h), read against the
surface call (vxrt_voxelize_mesh_device) on the same mesh in the same process: the project had no solid route before, so that is the
yardstick.  Prints one JSON document (profiles/solid/).

Cases: an icosphere at 4 and 6 subdivisions (5 120 and 81 920 triangles) with radii 10, 100 and 1 000 voxels (--radii picks fewer:
the largest holds 4.2 G interior cells, close to the call's 2^32 limit, and needs some 140 GB of scratch and output).  Per case and
mode (union, interior), host clock around the synchronous call with the mesh already on the device, after one warm-up, median / min /
max over the repeats: "count" (pos == mrgb == NULL) and "fetch" (one run into arrays with room to spare); "surface" holds the same
two for vxrt_voxelize_mesh_device.  A call the library refuses is recorded with its status and message.
  --device-only   only the solid fetch calls (the kernel-trace run):
                  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/solid_latency.py --device-only --calls DIR/calls.json
  --summarize DIR per-call kernel time of those calls, split into the surface stages (the vox_* kernels but the decode), the crossing
                  stages (columns, count, emit), the crossing sort, the fill (pairs and fill), the final sort (with the dedupe) and
                  the decode"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_voxel_raytracer_amd import Context  # noqa: E402
from voxelize_latency import DEV, icosphere, stats_ms, sync_timed  # noqa: E402

SURFACE = ("vox_setup_kernel", "vox_reduce_kernel", "vox_offsets_kernel", "vox_walk_kernel")
CROSSING = ("solid_columns_kernel", "solid_cross_kernel")
FILL_STAGE = ("solid_pairs_kernel", "solid_split_kernel", "solid_open_kernel", "solid_fill_kernel")
RADIX = ("radix_hist_kernel", "radix_scan_kernel", "radix_scatter_kernel")
DEDUPE = ("flag_count_kernel", "dedupe_write_kernel")
KERNELS = SURFACE + CROSSING + FILL_STAGE + RADIX + DEDUPE + ("solid_spread_kernel", "exclusive_scan_kernel", "vox_decode_kernel")
STAGES = ("surface", "crossing", "crossing_sort", "fill", "final_sort", "decode")
FILL = (7, 0x40, 0x80, 0xC0)
MODES = (("union", 0), ("interior", 1))


def run(repeats, device_only, calls, radii):
    out = {}
    fill = (C.c_uint8 * 4)(*FILL)
    with Context(64, 64) as ctx:
        L = ctx._L
        for sub in (4, 6):
            for radius in radii:
                v, t = icosphere(sub, float(radius))
                name = f"icosphere {sub}, radius {radius}"
                k = np.arange(len(t))
                m = np.stack([k % 128, k % 256, (k // 7) % 256, (k // 256) % 256], axis=1).astype(np.uint8)
                dv, dt, dm = torch.as_tensor(v, device=DEV), torch.as_tensor(t.view(np.int32), device=DEV), torch.as_tensor(m, device=DEV)
                mesh = (ctx._h, C.c_void_p(dv.data_ptr()), C.c_size_t(len(dv)), C.c_void_p(dt.data_ptr()), C.c_void_p(dm.data_ptr()), C.c_size_t(len(dt)))
                got = C.c_size_t(0)
                case = {"triangles": int(len(t))}

                def timed(what, count_call, fetch_call):
                    """count_call() / fetch_call(pos, mrgb, cap) -> status; -> {"voxels", "count", "fetch"} or the refusal"""
                    rc = count_call()
                    if rc != 0:
                        return {"refused": rc, "message": (L.vxrt_last_error() or b"").decode()}
                    n = int(got.value)
                    try:
                        pos, mrgb = torch.empty((n + 16, 3), dtype=torch.int16, device=DEV), torch.empty((n + 16, 4), dtype=torch.uint8, device=DEV)
                    except RuntimeError as e:
                        return {"voxels": n, "refused": "no room for the result", "message": str(e).splitlines()[0]}
                    samples = {"count": [], "fetch": []}
                    for r in range(repeats + 1):
                        todo = (("fetch", lambda: fetch_call(pos, mrgb, n + 16)),) if device_only else (("count", count_call), ("fetch", lambda: fetch_call(pos, mrgb, n + 16)))
                        for kind, fn in todo:
                            dt_s, rc = sync_timed(fn)
                            if rc != 0:
                                return {"voxels": n, "refused": rc, "message": (L.vxrt_last_error() or b"").decode()}
                            assert got.value == n
                            if r:
                                samples[kind].append(dt_s)
                        if what != "surface":
                            calls.append([f"{name}, {what}", "timed" if r else "warm"])
                    return {"voxels": n, **{kind: stats_ms(s) for kind, s in samples.items() if s}}

                if not device_only:
                    case["surface"] = timed("surface", lambda: L.vxrt_voxelize_mesh_device(*mesh, None, None, C.c_size_t(0), C.byref(got)),
                                            lambda p, o, cap: L.vxrt_voxelize_mesh_device(*mesh, C.c_void_p(p.data_ptr()), C.c_void_p(o.data_ptr()),
                                                                                          C.c_size_t(cap), C.byref(got)))
                for what, mode in MODES:
                    case[what] = timed(what, lambda: L.vxrt_voxelize_solid_device(*mesh, fill, C.c_uint32(mode), None, None, C.c_size_t(0), C.byref(got)),
                                       lambda p, o, cap: L.vxrt_voxelize_solid_device(*mesh, fill, C.c_uint32(mode), C.c_void_p(p.data_ptr()),
                                                                                      C.c_void_p(o.data_ptr()), C.c_size_t(cap), C.byref(got)))
                    torch.cuda.empty_cache()
                out[name] = case
                print(json.dumps({name: case}), file=sys.stderr, flush=True)
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
    groups = [g for g in groups if any(r[2] == "vox_decode_kernel" for r in g)]       # the fetch calls (each case counts once first)
    assert len(groups) == len(calls), (len(groups), len(calls))
    out = {}
    for (case, kind), g in zip(calls, groups):
        if kind != "timed":
            continue
        c = out.setdefault(case, {"stages": {w: [] for w in STAGES}, "per_kernel_us": {}})
        part = dict.fromkeys(STAGES, 0)
        paired, where = False, "surface"
        for s, e, k in g:
            paired |= k == "solid_pairs_kernel"
            if k in SURFACE:
                where = "surface"
            elif k in CROSSING:
                where = "crossing"
            elif k in FILL_STAGE:
                where = "fill"
            elif k in RADIX:
                where = "final_sort" if paired else "crossing_sort"
            elif k in DEDUPE:
                where = "final_sort"
            elif k == "vox_decode_kernel":
                where = "decode"
            # solid_spread_kernel and exclusive_scan_kernel belong to the stage of the kernel before them
            part[where] += e - s
            c["per_kernel_us"].setdefault(k, []).append((e - s) / 1e3)
        for w, ns in part.items():
            c["stages"][w].append(ns / 1e6)
    return {case: {"calls": len(c["stages"]["surface"]),
                   **{w: {"median_ms": float(np.median(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))} for w, v in c["stages"].items()},
                   "per_kernel_us_per_call": {k: float(np.sum(v)) / len(c["stages"]["surface"]) for k, v in c["per_kernel_us"].items()}}
            for case, c in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--radii", type=int, nargs="+", default=[10, 100, 1000])
    ap.add_argument("--calls", help="write the list of fetch calls here (for --summarize)")
    ap.add_argument("--summarize")
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.summarize:
        result = summarize(args.summarize)
    else:
        calls = []
        result = run(args.repeats, args.device_only, calls, args.radii)
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
