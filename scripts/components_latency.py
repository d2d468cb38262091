"""Latency of labelling connected components on the device (vxrt_label_components_device, vxrt_detached_voxels_device,
include/vxrt_components.h), read against the only route the project had before: vxrt_get_voxels to the host and a flood fill on the
CPU (tests/components_model.py, pure Python over a dict).  Prints one JSON document (profiles/components/).

Cases: the voxel lists of menger.vox and monu10.vox (tests/golden/scenes/) and a 128^3 random grid at occupancy 0.31, each labelled
at connectivity 6 and 26 with the list already on the device; detached_voxels of menger.vox and monu10.vox loaded as scenes, the
anchor box their lowest y layer, count and fetch.  Host clock around the synchronous call, after one warm-up, median / min / max over
the repeats.  "host_route" holds the comparison, timed once per case (it takes seconds to minutes): get_voxels, then the model.
  --no-host-route   leave the comparison out
  --grid N          side of the random grid (default 128)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import components_model as K  # noqa: E402
from gpu_voxel_raytracer_amd import Context, scenes  # noqa: E402
from voxelize_latency import DEV, stats_ms, sync_timed  # noqa: E402

CONNECTIVITIES = (6, 26)


def label_case(ctx, pos, repeats, host_route):
    L = ctx._L
    d_pos = torch.as_tensor(np.ascontiguousarray(pos, np.int16), device=DEV)
    label = torch.empty(len(pos), dtype=torch.int32, device=DEV)
    got = C.c_size_t(0)
    case = {"entries": int(len(pos))}
    for conn in CONNECTIVITIES:
        samples = {"count": [], "label": []}
        for r in range(repeats + 1):
            for kind, out in (("count", None), ("label", C.c_void_p(label.data_ptr()))):
                dt, rc = sync_timed(lambda: L.vxrt_label_components_device(ctx._h, C.c_void_p(d_pos.data_ptr()), C.c_size_t(len(pos)), C.c_uint32(conn),
                                                                           out, C.byref(got)))
                assert rc == 0, (L.vxrt_last_error() or b"").decode()
                if r:
                    samples[kind].append(dt)
        entry = {"components": int(got.value), **{kind: stats_ms(s) for kind, s in samples.items()}}
        if host_route:
            t0 = time.perf_counter()
            want, count = K.label(pos, conn)
            entry["host_route"] = {"model_s": time.perf_counter() - t0}
            assert count == got.value and np.array_equal(label.cpu().numpy().view(np.uint32), want)
        case[f"connectivity {conn}"] = entry
    return case


def scene_case(ctx, pos, mrgb, repeats, host_route):
    L = ctx._L
    ctx.recreate_octree(pos, mrgb)
    lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
    anchor = ((C.c_int32 * 3)(*lo.tolist()), (C.c_int32 * 3)(int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))
    got = C.c_size_t(0)
    case = {"voxels": int(len(pos))}
    out_pos, out_mrgb = torch.empty((len(pos), 3), dtype=torch.int16, device=DEV), torch.empty((len(pos), 4), dtype=torch.uint8, device=DEV)
    for conn in CONNECTIVITIES:
        samples = {"count": [], "fetch": []}
        for r in range(repeats + 1):
            for kind, arrays in (("count", (None, None, C.c_size_t(0))),
                                 ("fetch", (C.c_void_p(out_pos.data_ptr()), C.c_void_p(out_mrgb.data_ptr()), C.c_size_t(len(pos))))):
                dt, rc = sync_timed(lambda: L.vxrt_detached_voxels_device(ctx._h, anchor[0], anchor[1], C.c_uint32(conn), *arrays, C.byref(got)))
                assert rc == 0, (L.vxrt_last_error() or b"").decode()
                if r:
                    samples[kind].append(dt)
        entry = {"detached": int(got.value), **{kind: stats_ms(s) for kind, s in samples.items()}}
        if host_route:
            t0 = time.perf_counter()
            hp, hm = ctx.get_voxels()
            t1 = time.perf_counter()
            want = K.detached({tuple(p): tuple(b) for p, b in zip(hp.tolist(), hm.tolist())}, list(anchor[0]), list(anchor[1]), conn)
            entry["host_route"] = {"get_voxels_s": t1 - t0, "model_s": time.perf_counter() - t1}
            assert len(want[0]) == got.value and np.array_equal(out_pos[:got.value].cpu().numpy(), want[0])
        case[f"connectivity {conn}"] = entry
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    result = {"label_components": {}, "detached_voxels": {}}
    with Context(64, 64) as ctx:
        lists = {name + ".vox": scenes.load_scene(name)[:2] for name in ("menger", "monu10")}
        for name, (pos, mrgb) in lists.items():
            result["label_components"][name] = label_case(ctx, pos, args.repeats, not args.no_host_route)
            print(json.dumps({name: result["label_components"][name]}), file=sys.stderr, flush=True)
        grid = np.argwhere(np.random.default_rng(1).random((args.grid,) * 3) < 0.31) - args.grid // 2
        name = f"random {args.grid}^3 at 0.31"
        result["label_components"][name] = label_case(ctx, grid, args.repeats, False)      # the model would take minutes here
        print(json.dumps({name: result["label_components"][name]}), file=sys.stderr, flush=True)
        for name, (pos, mrgb) in lists.items():
            result["detached_voxels"][name] = scene_case(ctx, pos, mrgb, args.repeats, not args.no_host_route)
            print(json.dumps({name: result["detached_voxels"][name]}), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
