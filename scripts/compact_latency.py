"""What vxrt_compact_scene costs and what it buys (include/vxrt_compact.h; results under profiles/compact/).  One mode per run, each
printing one JSON document:

  --mode compact   host clock around compact_scene(), warmed, median / min / max over the repeats, on menger.vox and BASELINE config
                   5's sponge, each after 10^5 random edits (half sets, half clears, in the scene's box) and after 1000
                   clear-and-set cycles of an aligned 16^3 box; the scene is loaded and edited anew for every repeat.  Also the
                   storage before and after, and the bytes the relayout has to move (each live record and leaf word read and
                   written once).  --calls FILE lists the calls for --summarize.
  --mode route     the rebuild a host had before: get_voxels_device() then set_voxels_device() on the same edited scenes.  Needs
                   nothing of this extension, so it runs with any build of the library (VXRT_LIB).
  --mode growth    scene_storage() after each of 1000 cycles on menger.vox, with and without a compaction every 100 cycles.
  --mode frames    the bench frame's trace stage (menger.vox, 1920 x 1080, 4 bounces, TIMED) on the edited scene, the compacted one
                   and a fresh build of the same voxels, the three contexts taking turns block by block.
  --summarize DIR  per-call kernel time from a `rocprofv3 --kernel-trace --stats -d DIR -- python scripts/compact_latency.py --mode
                   compact --calls DIR/calls.json` run."""
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
from gpu_voxel_raytracer_amd import TIMED, TRACE, Camera, Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.scenes import CONFIG5  # noqa: E402

DEV = torch.device("cuda", 0)
KERNELS = ("compact_count_kernel", "exclusive_scan_kernel", "compact_expand_kernel")
BOX = 16


def stats_ms(samples):
    s = np.asarray(samples) * 1e3
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "n": int(len(s))}


def timed(fn):
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(DEV)
    return time.perf_counter() - t0


def loaders():
    pos, mrgb, _ = scenes.load_scene("menger")
    lo, hi = pos.min(0), pos.max(0)
    return {"menger.vox": (lambda c: c.recreate_octree(pos, mrgb), lo, hi, (32, 32, 32)),
            "config5": (lambda c: c.set_menger(*CONFIG5), np.zeros(3, int), np.full(3, CONFIG5[1] - 1), (1024, 1024, 1024))}


def box_list(origin):
    cells = np.array([np.array(origin) + np.array(p) for p in np.ndindex(BOX, BOX, BOX)], np.int16)
    colours = np.random.default_rng(9).integers(0, 256, (len(cells), 4)).astype(np.uint8)
    return torch.as_tensor(cells, device=DEV), torch.as_tensor(colours, device=DEV)


def random_edits(ctx, lo, hi, n=100000):
    """§9's 10^5 random edits: half sets with random colours, half clears, uniformly in the scene's box."""
    rng = np.random.default_rng(1)
    sets = rng.integers(lo, hi + 1, size=(n // 2, 3)).astype(np.int16)
    ctx.edit_voxels_device(torch.as_tensor(sets, device=DEV), torch.as_tensor(rng.integers(0, 256, size=(n // 2, 4)).astype(np.uint8), device=DEV))
    ctx.clear_voxels_device(torch.as_tensor(rng.integers(lo, hi + 1, size=(n - n // 2, 3)).astype(np.int16), device=DEV))


def cycles(ctx, origin, n=1000, each=None):
    cells, colours = box_list(origin)
    for k in range(n):
        ctx.clear_voxels_device(cells)
        ctx.edit_voxels_device(cells, colours)
        if each:
            each(k)


def damages(lo, hi, origin):
    return {"1e5 random edits": lambda c: random_edits(c, lo, hi), "1000 cycles of a 16^3 box": lambda c: cycles(c, origin)}


def mode_compact(args):
    out, calls = {"device": torch.cuda.get_device_name(DEV), "cases": []}, []
    for scene, (load, lo, hi, origin) in loaders().items():
        if scene == "config5" and args.skip_config5:
            continue
        for what, damage in damages(lo, hi, origin).items():
            samples, row = [], {"scene": scene, "after": what}
            with Context(64, 64) as ctx:
                for k in range(args.repeats + 1):          # the first is the warm-up
                    load(ctx)
                    damage(ctx)
                    before = ctx.scene_storage()
                    dt = timed(ctx.compact_scene)
                    after = ctx.scene_storage()
                    calls.append({"scene": scene, "after": what, "levels": ctx.scene_depth + 1, "warmup": k == 0})
                    if k:
                        samples.append(dt)
                row.update({"depth": ctx.scene_depth, "storage_before": before, "storage_after": after, "compact_scene": stats_ms(samples)})
                # read and written once: every live record and leaf word
                moved = 2 * (8 * after["records_live"] + 4 * after["leaves_used"])
                row["bytes_moved"] = moved
                row["bytes_per_s_of_the_call"] = moved / (row["compact_scene"]["median_ms"] * 1e-3)
            out["cases"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    if args.calls:
        with open(args.calls, "w") as f:
            json.dump({"calls": calls}, f)
    return out


def mode_route(args):
    out = {"device": torch.cuda.get_device_name(DEV), "library": os.path.basename(os.environ.get("VXRT_LIB", "the tree's")), "cases": []}
    for scene, (load, lo, hi, origin) in loaders().items():
        if scene == "config5" and args.skip_config5:
            continue
        for what, damage in damages(lo, hi, origin).items():
            samples, row = [], {"scene": scene, "after": what}
            with Context(64, 64) as ctx:
                for k in range((min(args.repeats, 3) if scene == "config5" else args.repeats) + 1):
                    load(ctx)
                    damage(ctx)

                    def route():
                        pos, mrgb = ctx.get_voxels_device()
                        ctx.set_voxels_device(pos, mrgb)
                    dt = timed(route)
                    if k:
                        samples.append(dt)
                row.update({"voxels": int(ctx.count_voxels()), "get_voxels_device_then_set_voxels_device": stats_ms(samples)})
            torch.cuda.empty_cache()
            out["cases"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    if not args.skip_config5:
        with Context(64, 64) as ctx:
            ctx.set_menger(*CONFIG5)
            out["config5_set_menger"] = stats_ms([timed(lambda: ctx.set_menger(*CONFIG5)) for _ in range(3)])
    return out


def mode_growth(args):
    load, lo, hi, origin = loaders()["menger.vox"]
    out = {"scene": "menger.vox", "cycles": 1000, "box": BOX, "compaction_every": 100}
    for label, every in (("without", 0), ("with", 100)):
        rows = []
        with Context(64, 64) as ctx:
            load(ctx)
            built = ctx.scene_storage()

            def each(k):
                if every and (k + 1) % every == 0:
                    ctx.compact_scene()
                s = ctx.scene_storage()
                rows.append([s["records_live"], s["records_used"], s["records_capacity"], s["leaves_used"], s["leaves_capacity"]])
            cycles(ctx, origin, each=each)
        a = np.array(rows, np.int64)
        used = 8 * a[:, 1] + 4 * a[:, 3]
        cap = 8 * a[:, 2] + 4 * a[:, 4]
        out[label] = {"as_built": built, "after_cycle_1": rows[0], "after_cycle_1000": rows[-1],
                      "bytes_in_use_per_cycle": float(np.median(np.diff(used)[np.diff(used) > 0])) if every == 0 else None,
                      "peak_bytes_in_use": int(used.max()), "peak_bytes_allocated": int(cap.max()),
                      "fields": ["records_live", "records_used", "records_capacity", "leaves_used", "leaves_capacity"],
                      "every_50th_cycle": rows[49::50]}
    return out


def mode_frames(args):
    pos, mrgb, size = scenes.load_scene("menger")
    cam = Camera(*scenes.bench_camera(size))
    lo, hi = pos.min(0), pos.max(0)
    names = ("edited", "compacted", "fresh")
    ctxs = {n: Context(1920, 1080, max_bounces=4) for n in names}
    try:
        for n in ("edited", "compacted"):
            ctxs[n].recreate_octree(pos, mrgb)
            random_edits(ctxs[n], lo, hi)
            cycles(ctxs[n], (32, 32, 32))
        ctxs["compacted"].compact_scene()
        ctxs["fresh"].recreate_octree(*ctxs["edited"].get_voxels())
        per = {n: [] for n in names}
        for c in ctxs.values():
            c.camera = cam
            c.render_frames(TRACE, args.frames)   # warm-up
            c.sync()
        for _ in range(args.blocks):
            for n in names:                        # taking turns: what else runs on the machine hits all three alike
                c = ctxs[n]
                c.reset_stats()
                c.render_frames(TRACE | TIMED, args.frames)
                c.sync()
                st = c.stats()
                per[n].append(st.trace_ms / max(1, st.timed_frames))
        same = all(np.array_equal(ctxs["edited"].read(i), ctxs[n].read(i)) for n in ("compacted", "fresh") for i in (0, 1))
        return {"device": torch.cuda.get_device_name(DEV),
                "workload": f"menger.vox after 10^5 random edits and 1000 box cycles, 1920x1080, 4 bounces, trace stage (TIMED), {args.blocks} blocks of {args.frames} frames, the contexts alternating",
                "identical_images": bool(same),
                "storage": {n: ctxs[n].scene_storage() for n in names},
                "trace_ms_per_frame": {n: {"median": float(np.median(per[n])), "min": float(np.min(per[n])), "max": float(np.max(per[n])),
                                           "blocks": [round(float(v), 4) for v in per[n]]} for n in names}}
    finally:
        for c in ctxs.values():
            c.close()


def summarize(root):
    meta = json.load(open(os.path.join(root, "calls.json")))
    found = []
    for f in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            found += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows = sorted((s, e, next(n for n in KERNELS if n in k)) for s, e, k in found if "compact_count_kernel" in k or "compact_expand_kernel" in k)
    scans = sorted((s, e) for s, e, k in found if "exclusive_scan_kernel" in k)
    # every call of L levels is L count and L expand launches, in the order of calls.json
    assert len(rows) == sum(2 * c["levels"] for c in meta["calls"]), (len(rows), len(meta["calls"]))
    cases, at = {}, 0
    for call in meta["calls"]:
        mine, at = rows[at:at + 2 * call["levels"]], at + 2 * call["levels"]
        if call["warmup"]:
            continue
        t0, t1 = mine[0][0], mine[-1][1]
        per = {k: sum(e - s for s, e, n in mine if n == k) * 1e-6 for k in ("compact_count_kernel", "compact_expand_kernel")}
        per["exclusive_scan_kernel"] = sum(e - s for s, e in scans if t0 <= s <= t1) * 1e-6
        per["first_kernel_to_last_ms"] = (t1 - t0) * 1e-6
        cases.setdefault((call["scene"], call["after"]), []).append(per)
    out = []
    for (scene, after), calls in cases.items():
        sums = [sum(c[k] for k in KERNELS) for c in calls]
        out.append({"scene": scene, "after": after, "calls": len(calls), "kernels_ms_median": float(np.median(sums)), "kernels_ms_min": float(min(sums)),
                    "kernels_ms_max": float(max(sums)), "per_kernel_ms_median": {k: float(np.median([c[k] for c in calls])) for k in KERNELS},
                    "first_kernel_to_last_ms_median": float(np.median([c["first_kernel_to_last_ms"] for c in calls]))})
    return {"cases": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("compact", "route", "growth", "frames"), default="compact")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--skip-config5", action="store_true")
    ap.add_argument("--calls", help="write the list of compaction calls here (for --summarize)")
    ap.add_argument("--summarize")
    ap.add_argument("--out")
    args = ap.parse_args()
    result = summarize(args.summarize) if args.summarize else {"compact": mode_compact, "route": mode_route, "growth": mode_growth, "frames": mode_frames}[args.mode](args)
    text = json.dumps(result, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
