"""Latency of in-place scene edits (vxrt_edit_voxels) against a rebuild (vxrt_set_voxels of the whole edited list), and the frame time
of the bench scene after many edits against a fresh build of the same voxels.  Prints one JSON document (profiles/edit/).

Latency: a host clock around the synchronous call, warmed (one call first), median / min / max over repeats; random sets and clears
inside the scene's bounding box, batches of 1 .. 2^20.  Scenes: menger.vox, monu10.vox and the device-built sponge of BASELINE
config 5 (vxrt_set_menger; no host list exists, so its "rebuild" is vxrt_set_menger itself).
  --quick          small batches and few repeats only (the kernel-trace run: rocprofv3 --kernel-trace --stats -- python ...)
  --frame-edits N  random edits before the frame-time comparison (default 10^5)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_voxel_raytracer_amd import ALL, Camera, Context, scenes  # noqa: E402


def stats_ms(samples):
    s = np.asarray(samples) * 1e3
    return {"median_ms": float(np.median(s)), "min_ms": float(s.min()), "max_ms": float(s.max()), "n": int(len(s))}


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def latency(ctx, lo, hi, existing, sizes, repeats, rng, rebuild):
    out = []
    for n in sizes:
        row = {"batch": n}
        for kind in ("set", "clear"):
            samples = []
            for r in range(repeats(n) + 1):   # the first call warms
                if kind == "set":
                    pos = rng.integers(lo, hi + 1, size=(n, 3)).astype(np.int16)
                    mrgb = rng.integers(0, 256, size=(n, 4)).astype(np.uint8)
                    dt = timed(lambda: ctx.edit_voxels(pos, mrgb))
                else:
                    pos = existing[rng.integers(0, len(existing), size=n)] if existing is not None else \
                        rng.integers(lo, hi + 1, size=(n, 3)).astype(np.int16)
                    dt = timed(lambda: ctx.clear_voxels(pos))
                if r:
                    samples.append(dt)
            row[kind] = stats_ms(samples)
        row["rebuild"] = rebuild(n)
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--frame-edits", type=int, default=100000)
    ap.add_argument("--skip-config5", action="store_true")
    ap.add_argument("--out", help="also write the JSON document here")
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    sizes = [1, 64, 4096] if args.quick else [1, 64, 4096, 1 << 17, 1 << 20]
    repeats = (lambda n: 3) if args.quick else (lambda n: 30 if n <= 4096 else (5 if n <= (1 << 17) else 3))
    result = {"sizes": sizes, "scenes": {}}

    for name in ("menger", "monu10"):
        pos, mrgb, size = scenes.load_scene(name)
        lo, hi = pos.min(0), pos.max(0)
        with Context(256, 256, max_bounces=4) as ctx:
            ctx.recreate_octree(pos, mrgb)

            def rebuild(n):
                extra = rng.integers(lo, hi + 1, size=(n, 3)).astype(np.int16)
                p = np.concatenate([pos, extra])
                m = np.concatenate([mrgb, rng.integers(0, 256, size=(n, 4)).astype(np.uint8)])
                with Context(64, 64) as other:
                    other.recreate_octree(pos, mrgb)
                    return stats_ms([timed(lambda: other.recreate_octree(p, m)) for _ in range(3)])
            result["scenes"][name] = {"voxels": int(len(pos)), "latency": latency(ctx, lo, hi, pos, sizes, repeats, rng, rebuild)}

    if not args.skip_config5:
        level, clip, colour, period = scenes.CONFIG5
        with Context(256, 256, max_bounces=4) as ctx:
            t_build = [timed(lambda: ctx.set_menger(level, clip, colour, period)) for _ in range(2)]
            st = ctx.stats()
            result["scenes"]["config5_device_menger"] = {
                "records": int(st.octree_nodes), "scene_bytes": int(st.scene_bytes),
                "latency": latency(ctx, 0, clip - 1, None, sizes, repeats, rng, lambda n: {"set_menger": stats_ms(t_build)})}

    # frame time of the bench scene (menger 1080p, 4 bounces) after many random edits, against a fresh build of the same voxels
    if not args.quick:
        pos, mrgb, size = scenes.load_scene("menger")
        cam = scenes.bench_camera(size)
        lo, hi = pos.min(0), pos.max(0)
        frames = {}
        with Context(1920, 1080, max_bounces=4) as ctx:
            ctx.recreate_octree(pos, mrgb)
            n = args.frame_edits
            sets = rng.integers(lo, hi + 1, size=(n // 2, 3)).astype(np.int16)
            ctx.edit_voxels(sets, rng.integers(0, 256, size=(n // 2, 4)).astype(np.uint8))
            ctx.clear_voxels(rng.integers(lo, hi + 1, size=(n - n // 2, 3)).astype(np.int16))
            svo, leaves = ctx.read_scene()
            st = ctx.stats()
            frames["edited"] = {"records_in_use": int(len(svo)), "live_records": int(st.octree_nodes), "scene_bytes": int(st.scene_bytes)}
            voxels = decode(svo, leaves, st.octree_depth)
            for label, c in (("edited", ctx),):
                frames[label].update(frame_time(c, cam))
        with Context(1920, 1080, max_bounces=4) as ref:
            ref.recreate_octree(*voxels)
            frames["fresh"] = {"records_in_use": int(ref.stats().octree_nodes), **frame_time(ref, cam)}
        frames["edits"] = args.frame_edits
        result["frame_after_edits"] = frames
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


def frame_time(ctx, cam, frames=40, reps=5):
    ctx.camera = Camera(*cam)
    ctx.render_frames(ALL, 8)
    ctx.sync()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        ctx.render_frames(ALL, frames)
        ctx.sync()
        per.append((time.perf_counter() - t0) / frames)
    return {"frame": stats_ms(per)}


POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int64)


def decode(svo, leaves, depth):
    """The device records -> voxel list (pos, mrgb), following the pointers from the root."""
    idx = np.zeros(1, np.int64)
    u = np.zeros((1, 3), np.int64)
    for level in range(depth + 1):
        rec = svo[idx]
        masks = (rec[:, 0].astype(np.int64) >> (8 if level == depth else 0)) & 0xFF
        nidx, nu = [], []
        for s in range(8):
            has = (masks >> s) & 1 == 1
            rank = POPCOUNT[masks[has] & ((1 << s) - 1)]
            nidx.append(rec[has, 1].astype(np.int64) + rank)
            nu.append(u[has] * 2 + np.array([(s >> 2) & 1, (s >> 1) & 1, s & 1]))
        idx, u = np.concatenate(nidx), np.concatenate(nu)
    w = leaves[idx].astype(np.uint32)
    mrgb = np.stack([(w >> 24) & 0x7F, (w >> 16) & 0xFF, (w >> 8) & 0xFF, w & 0xFF], 1).astype(np.uint8)
    return (u - (1 << depth)).astype(np.int16), mrgb


if __name__ == "__main__":
    main()
