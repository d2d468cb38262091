"""What taking every frame to the host costs in the reference's own loop, rgba32f against the displayed frame's 4 bytes per pixel.

The loop (bench.py's scene: vox/menger.vox, 1920x1080, MAX_BOUNCES 4): per frame vxrt_set_camera (an orbiting camera, as bench.py's
reference loop moves it) and vxrt_render(VXRT_ALL), denoise radius 2, frames_in_flight 2.  Three variants, alternated block by block in
one process (--inflight 1: the same with one frame in flight):
  a  no read-back (one sync at the end of a block);
  b  vxrt_read_async(VXRT_DENOISED) into two pinned slots: frame f goes to slot f & 1, the host waits for frame f - 1's slot;
  c  the same with vxrt_read_async(VXRT_DISPLAY_BGRA8_SRGB) (the sRGB encode on the GPU, 4 bytes per pixel).
Each block runs for at least --block-s seconds; the figure is the median over --blocks blocks, with the spread (min, max).  The transfer
alone (slot by slot, nothing rendering) is measured for both formats too.

    python scripts/display_readback.py --out profiles/display/readback_inflight2.json

--encode-only N: N encodes of one frame (vxrt_device_image(VXRT_DISPLAY_BGRA8_SRGB)) and nothing else — the run to put under
`rocprofv3 --kernel-trace --stats` for the kernel's own time.  --stats <kernel_stats.csv>: summarise such a run (the encode kernel's
mean time and its achieved bytes/s at 20 bytes per pixel: a 16-byte load and a 4-byte store)."""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BOUNCES, RADIUS, SCENE = 1920, 1080, 4, 2, "menger"


def make_context(device=0, inflight=2):
    from gpu_voxel_raytracer_amd import Context, scenes
    pos, mrgb, size = scenes.load_scene(SCENE)
    ctx = Context(W, H, device=device, max_bounces=BOUNCES, frames_in_flight=inflight)
    ctx.recreate_octree(pos, mrgb)
    ctx.denoise_uniforms.radius = RADIUS
    return ctx, size


def measure(args):
    from gpu_voxel_raytracer_amd import ALL, DENOISED, DISPLAY_BGRA8_SRGB, Camera
    from gpu_voxel_raytracer_amd.frame_loop import orbit_camera
    ctx, size = make_context(args.device, args.inflight)
    path = [orbit_camera(size, 0.62 + 0.25 * f / 960.0) for f in range(960)]
    slots = {DENOISED: [ctx.pinned_image(), ctx.pinned_image()], DISPLAY_BGRA8_SRGB: [ctx.pinned_display(), ctx.pinned_display()]}
    frame = [0]

    def render():
        ctx.camera = Camera(*path[frame[0] % len(path)])
        ctx.render(ALL)
        frame[0] += 1

    def block(which, seconds):
        """frames of the loop until `seconds` have passed; -> ms per frame (the drain at the end included)"""
        n = 0
        t0 = time.perf_counter()
        while True:
            render()
            if which is not None:
                ctx.read_async(which, slots[which][n & 1], n & 1)
                if n >= 1:
                    ctx.read_wait((n + 1) & 1)       # frame n - 1 has arrived: the host may show or store it
            n += 1
            if n % 8 == 0 and time.perf_counter() - t0 >= seconds:
                break
        if which is None:
            ctx.sync()
        else:
            ctx.read_wait(0)
            ctx.read_wait(1)
        return (time.perf_counter() - t0) / n * 1e3, n

    variants = {"a_no_readback": None, "b_read_async_rgba32f": DENOISED, "c_read_async_display_bgra8": DISPLAY_BGRA8_SRGB}
    for name, which in variants.items():      # warm-up: queues, pinned pages, the first encode
        block(which, 0.3)
    results = {name: [] for name in variants}
    for _ in range(args.blocks):
        for name, which in variants.items():
            ms, n = block(which, args.block_s)
            results[name].append({"ms_per_frame": round(ms, 4), "frames": n})
    summary = {}
    for name, runs in results.items():
        ms = sorted(r["ms_per_frame"] for r in runs)
        summary[name] = {"median_ms_per_frame": ms[len(ms) // 2], "min_ms_per_frame": ms[0], "max_ms_per_frame": ms[-1],
                         "spread_pct": round((ms[-1] - ms[0]) / ms[len(ms) // 2] * 100, 2), "blocks": runs}
    transfer = {}
    ctx.sync()
    for name, which in (("rgba32f", DENOISED), ("display_bgra8", DISPLAY_BGRA8_SRGB)):
        buf = slots[which]
        for k in range(4):
            ctx.read_async(which, buf[k & 1], k & 1)
            ctx.read_wait(k & 1)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            for k in range(32):
                ctx.read_async(which, buf[k & 1], k & 1)
                ctx.read_wait(k & 1)
            t.append((time.perf_counter() - t0) / 32 * 1e3)
        ms = sorted(t)[2]
        nbytes = buf[0].array.nbytes
        transfer[name] = {"bytes": int(nbytes), "median_ms": round(ms, 4), "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)}
    for pair in slots.values():
        for b in pair:
            b.close()
    ctx.close()
    return {"workload": f"vox/{SCENE}.vox, {W}x{H}, MAX_BOUNCES {BOUNCES}, VXRT_ALL, denoise radius {RADIUS}, frames_in_flight {args.inflight}, "
                        "vxrt_set_camera every frame (orbit, 0.09 degrees per frame)",
            "method": f"variants alternated in one process; {args.blocks} blocks of >= {args.block_s} s each; median and spread of ms per frame",
            "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES", "unset"), "variants": summary, "transfer_alone": transfer}


def encode_only(args):
    from gpu_voxel_raytracer_amd import ALL, DISPLAY_BGRA8_SRGB, Camera, scenes
    ctx, size = make_context(args.device)
    ctx.camera = Camera(*scenes.bench_camera(size))
    ctx.render(ALL)
    ctx.sync()
    for _ in range(args.encode_only):
        ctx.device_image(DISPLAY_BGRA8_SRGB)
    ctx.sync()
    ctx.close()
    return {"encodes": args.encode_only, "pixels": W * H}


def stats(path):
    rows = [r for r in csv.DictReader(open(path)) if "display_encode_kernel" in r.get("Name", "")]
    if not rows:
        raise SystemExit(f"no display_encode_kernel in {path}")
    out = []
    for r in rows:
        mean_ns = float(r["AverageNs"])
        out.append({"kernel": r["Name"], "calls": int(r["Calls"]), "mean_us": round(mean_ns / 1e3, 2),
                    "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2),
                    "achieved_gb_per_s_at_20_bytes_per_pixel": round(20.0 * W * H / (mean_ns * 1e-9) / 1e9, 1)})
    return {"pixels": W * H, "bytes_moved_per_encode": 20 * W * H, "kernels": out}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--inflight", type=int, default=2, help="vxrt_config.frames_in_flight (the reference's loop as bench.py times it: 2)")
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--block-s", type=float, default=1.0)
    ap.add_argument("--encode-only", type=int, default=0)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.stats:
        res = stats(args.stats)
    elif args.encode_only:
        res = encode_only(args)
    else:
        res = measure(args)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
