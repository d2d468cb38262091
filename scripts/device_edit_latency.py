"""Latency of editing a loaded scene from a voxel list in device memory (vxrt_edit_voxels_device, include/vxrt_device_edit.h) against
the route a host had before it: the tensors' .cpu() plus vxrt_edit_voxels ("host").  Prints one JSON document (profiles/device_edit/).

Scenes: menger.vox and BASELINE config 5's sponge, built on the device (vxrt_set_menger(*CONFIG5)).  Cases: batches of 1, 64, 4096,
2^17 and 2^20 uniformly random positions of the root cube, set with random colours and then cleared again (the same list), so the
scene stays what it was but for the voxels the list happened to hit.  Every repeat draws a fresh list.  Both routes get the same
lists, each in a context of its own, and are checked to leave identical bytes.  Host clock around the synchronous call, after one
warm-up, median / min / max over the repeats; the lists are on the device before the clock starts.
Read side: a 256^3 box of config 5 through vxrt_get_voxels_device, against vxrt_get_voxels plus the upload of both arrays.
  --device-only   only the device-list calls (the kernel-trace run):
                  rocprofv3 --kernel-trace --stats -d DIR -- python scripts/device_edit_latency.py --device-only --calls DIR/calls.json
  --summarize DIR per-call kernel time of those calls (every call opens with edit_keys_kernel)"""
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
SIZES = (1, 64, 4096, 1 << 17, 1 << 20)
KERNELS = ("edit_keys_kernel", "edit_bounds_reduce_kernel", "radix_hist_kernel", "radix_scan_kernel", "radix_scatter_kernel",
           "flag_count_kernel", "exclusive_scan_kernel", "dedupe_write_kernel", "cut_count_kernel", "cut_offsets_kernel",
           "cut_write_kernel", "edit_kernel")


def stats_ms(samples):
    s = np.asarray(samples) * 1e3
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "n": int(len(s))}


def sync_timed(fn):
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(DEV)
    return time.perf_counter() - t0, out


def load(ctx, name):
    if name == "config5":
        ctx.set_menger(*CONFIG5)
    else:
        pos, mrgb, _ = scenes.load_scene(name)
        ctx.recreate_octree(pos, mrgb)


def host_set(ctx, pos, mrgb):
    ctx.edit_voxels(pos.cpu().numpy(), mrgb.cpu().numpy())


def host_clear(ctx, pos):
    ctx.clear_voxels(pos.cpu().numpy())


def run_scene(name, repeats, device_only, calls):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(9)
    out = {}
    with Context(64, 64) as a, Context(64, 64) as b:
        load(a, name)
        if not device_only:
            load(b, name)
        h = 1 << a.stats().octree_depth
        for n in SIZES:
            dev_set, dev_clear, host_s, host_c = [], [], [], []
            for r in range(repeats + 1):
                pos = torch.randint(-h, h, (n, 3), generator=gen, device=DEV, dtype=torch.int32).to(torch.int16)
                mrgb = torch.randint(0, 256, (n, 4), generator=gen, device=DEV, dtype=torch.int32).to(torch.uint8)
                ds, _ = sync_timed(lambda: a.edit_voxels_device(pos, mrgb))
                dc, _ = sync_timed(lambda: a.clear_voxels_device(pos))
                calls += [[f"{name} {n} set", "timed" if r else "warm"], [f"{name} {n} clear", "timed" if r else "warm"]]
                if not device_only:
                    hs, _ = sync_timed(lambda: host_set(b, pos, mrgb))
                    hc, _ = sync_timed(lambda: host_clear(b, pos))
                if r:
                    dev_set.append(ds)
                    dev_clear.append(dc)
                    if not device_only:
                        host_s.append(hs)
                        host_c.append(hc)
            row = {"set": {"edit_voxels_device": stats_ms(dev_set)}, "clear": {"edit_voxels_device": stats_ms(dev_clear)}}
            if not device_only:
                row["set"]["cpu_plus_edit_voxels"] = stats_ms(host_s)
                row["clear"]["cpu_plus_edit_voxels"] = stats_ms(host_c)
                if name != "config5" or n == SIZES[-1]:   # config 5's records are 6 GB: read back once, after the last case
                    sa, la = a.read_scene()
                    sb, lb = b.read_scene()
                    row["identical_bytes"] = bool(np.array_equal(sa, sb) and np.array_equal(la, lb))
            out[str(n)] = row
            print(json.dumps({name: {n: row}}), file=sys.stderr, flush=True)
        if not device_only and name == "config5":
            lo, hi = (0, 0, 0), (256, 256, 256)
            dev_t, host_t, count = [], [], 0
            for r in range(repeats + 1):
                dt, got = sync_timed(lambda: a.get_voxels_device(lo, hi))

                def host_route():
                    p, m = a.get_voxels(lo, hi)
                    return torch.as_tensor(p, device=DEV), torch.as_tensor(m, device=DEV)
                ht, want = sync_timed(host_route)
                count = len(got[0])
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
                if r:
                    dev_t.append(dt)
                    host_t.append(ht)
            out["read 256^3 box"] = {"voxels": count, "get_voxels_device": stats_ms(dev_t), "get_voxels_plus_upload": stats_ms(host_t)}
            print(json.dumps({name: {"read 256^3 box": out["read 256^3 box"]}}), file=sys.stderr, flush=True)
    return out


def summarize(root):
    calls = json.load(open(os.path.join(root, "calls.json")))
    found = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            found += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows = sorted((s, e, next(n for n in KERNELS if n in k)) for s, e, k in found if any(n in k for n in KERNELS))
    starts = [i for i, r in enumerate(rows) if r[2] == "edit_keys_kernel"]
    groups = [rows[a:b] for a, b in zip(starts, starts[1:] + [len(rows)])]
    # a call ends with its edit_kernel: what follows up to the next call (another scene's build) is not its own
    groups = [g[:1 + next(i for i, r in enumerate(g) if r[2] == "edit_kernel")] for g in groups]
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
                                                                       "min": float(np.min(c["busy_us"])) / 1e3,
                                                                       "max": float(np.max(c["busy_us"])) / 1e3},
                   "per_kernel_us_per_call": {k: float(np.sum(v)) / len(c["busy_us"]) for k, v in c["per_kernel_us"].items()}}
            for case, c in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--calls", help="write the list of device-edit calls here (for --summarize)")
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
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
