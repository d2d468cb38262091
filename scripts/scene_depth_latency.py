"""Latency of changing a loaded scene's octree depth in place (vxrt_set_scene_depth / vxrt_fit_scene_depth) against the rebuild a host
needed before (get_voxels -> set_voxels_device, or set_menger for the procedural sponge), and what an unfitted depth costs per frame.
Prints one JSON document (profiles/scene_depth/).

Scenes: menger.vox, the reference's start-up scene and BASELINE config 5's sponge (vxrt_set_menger(*CONFIG5)).  Calls: grow by 1,
shrink by 1 (back), grow to 15, fit (from one level above the rule's depth).  Host clock around the synchronous call, after a warm-up,
median / min / max over the repeats.  The first call on a scene that was never edited reallocates its storage (x 1.5); it is timed
on its own.  Frames: the bench frame (menger.vox, 1920 x 1080, 4 bounces, the trace stage, TIMED) at the rule's depth, +1, +4 and 15."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_voxel_raytracer_amd import TIMED, TRACE, Camera, Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.host import default_scene_voxels  # noqa: E402
from gpu_voxel_raytracer_amd.scenes import CONFIG5  # noqa: E402

DEV = torch.device("cuda", 0)


def stats_ms(samples):
    s = np.asarray(samples) * 1e3
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "n": int(len(s))}


def timed(fn):
    torch.cuda.synchronize(DEV)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize(DEV)
    return time.perf_counter() - t0


def depth_calls(ctx, repeats):
    d = ctx.scene_depth
    out = {"depth": d, "first_call_ms": timed(lambda: ctx.set_scene_depth(d + 1)) * 1e3}   # reallocates the never-edited storage
    ctx.set_scene_depth(d)
    for _ in range(2):   # warm-up
        ctx.set_scene_depth(d + 1)
        ctx.set_scene_depth(d)
    grow, shrink, top, fit = [], [], [], []
    for _ in range(repeats):
        grow.append(timed(lambda: ctx.set_scene_depth(d + 1)))
        shrink.append(timed(lambda: ctx.set_scene_depth(d)))
    for _ in range(repeats):
        top.append(timed(lambda: ctx.set_scene_depth(15)))
        ctx.set_scene_depth(d)
        ctx.set_scene_depth(d + 1)
        fit.append(timed(ctx.fit_scene_depth))
        assert ctx.scene_depth == d
    out.update({"grow_by_1": stats_ms(grow), "shrink_by_1": stats_ms(shrink), "grow_to_15": stats_ms(top), "fit_from_plus_1": stats_ms(fit),
                "scene_bytes_after": int(ctx.stats().scene_bytes), "octree_nodes": int(ctx.stats().octree_nodes)})
    return out


def rebuild_route(ctx, repeats):
    """get_voxels, then the device build from those lists"""
    samples = []
    for k in range(repeats + 1):
        def route():
            pos, mrgb = ctx.get_voxels()
            ctx.set_voxels_device(torch.from_numpy(pos).to(DEV), torch.from_numpy(mrgb).to(DEV))
        t = timed(route)
        if k:
            samples.append(t)
    return stats_ms(samples)


def frame_costs(blocks, frames):
    pos, mrgb, size = scenes.load_scene("menger")
    rows = []
    with Context(1920, 1080, max_bounces=4) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = Camera(*scenes.bench_camera(size))
        d = ctx.scene_depth
        for target in (d, d + 1, d + 4, 15):
            ctx.set_scene_depth(target)
            ctx.render_frames(TRACE, frames)   # warm-up
            ctx.sync()
            per_block = []
            for _ in range(blocks):
                ctx.reset_stats()
                ctx.render_frames(TRACE | TIMED, frames)
                ctx.sync()
                st = ctx.stats()
                per_block.append(st.trace_ms / max(1, st.timed_frames))
            rows.append({"depth": target, "levels_above_rule": target - d, "trace_ms_per_frame_median": float(np.median(per_block)),
                         "trace_ms_per_frame_blocks": [round(float(v), 4) for v in per_block]})
        ctx.set_scene_depth(d)
    return {"workload": f"menger.vox, 1920x1080, 4 bounces, trace stage (TIMED), {blocks} blocks of {frames} frames", "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--skip-config5", action="store_true")
    ap.add_argument("--skip-frames", action="store_true")
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(DEV), "scenes": {}}
    pos, mrgb, _ = scenes.load_scene("menger")
    for name, (p, m) in (("menger.vox", (pos, mrgb)), ("startup", default_scene_voxels(1))):
        with Context(64, 64) as ctx:
            ctx.recreate_octree(p, m)
            row = depth_calls(ctx, args.repeats)
            row["voxels"] = int(len(p))
            row["rebuild_get_voxels_set_voxels_device"] = rebuild_route(ctx, max(3, args.repeats // 4))
            out["scenes"][name] = row
        print(name, json.dumps(row), file=sys.stderr, flush=True)
    if not args.skip_config5:
        with Context(64, 64) as ctx:
            ctx.set_menger(*CONFIG5)
            row = depth_calls(ctx, args.repeats)
            samples = [timed(lambda: ctx.set_menger(*CONFIG5)) for _ in range(3)]
            row["rebuild_set_menger"] = stats_ms(samples)
            out["scenes"]["config5"] = row
        print("config5", json.dumps(row), file=sys.stderr, flush=True)
    if not args.skip_frames:
        out["frames"] = frame_costs(blocks=5, frames=16)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
