"""Latency of the device queries (vxrt_lookup_voxels_device, vxrt_pick_device, include/vxrt_query.h), read against the routes the
project offered before them, on the same machine in the same run.  Prints one JSON document (profiles/query/).

Lookup, on menger.vox and monu10.vox (tests/golden/scenes/) loaded as scenes, for three query lists already on the device: the scene's
own list (`own`), that list shifted by (1, 0, 0) (`shifted`) and 2^20 uniform random positions in the root cube (`random`): `lookup`
(Context.lookup_voxels: words and count), `count` (Context.count_present) and `torch_route`, the parent's route: get_voxels_device()
of the whole scene, keys for both lists in torch, a sort and searchsorted.
Rays: 2^20 rays through a camera's pixel centres (1024 x 1024, the bench camera): `pick_device` unbounded and with max_time = 4.0, the
rays already on the device, beside `pick` with the same rays from host arrays.
Host clock around the synchronous call, after one warm-up, median / min / max over the repeats.  The script asserts that the routes
agree: the words of both lookups, and the records of pick_device and pick byte for byte."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_voxel_raytracer_amd import Camera, Context, scenes  # noqa: E402
from gpu_voxel_raytracer_amd.host import PICK_HIT_DTYPE  # noqa: E402
from pieces_latency import timed  # noqa: E402
from voxelize_latency import DEV  # noqa: E402

RANDOM = 1 << 20
SIDE = 1024


def keys_of(pos):
    u = pos.to(torch.int64) + 32768
    return (u[:, 0] << 32) | (u[:, 1] << 16) | u[:, 2]


def torch_lookup(ctx, query, offset):
    """the parent's route to the same words: the whole scene extracted, both lists keyed, one sorted, the other searched in it"""
    pos, mrgb = ctx.get_voxels_device()
    m = mrgb.to(torch.int64)
    words = (0x80000000 | (m[:, 0] & 0x7F) << 24 | m[:, 1] << 16 | m[:, 2] << 8 | m[:, 3]).to(torch.int32)
    skeys, order = torch.sort(keys_of(pos))
    q = query.to(torch.int64) + torch.tensor(offset, dtype=torch.int64, device=query.device)
    ok = ((q >= -32768) & (q < 32768)).all(dim=1)
    qkeys = keys_of(q.clamp(-32768, 32767))
    at = torch.searchsorted(skeys, qkeys).clamp(max=len(skeys) - 1)
    found = ok & (skeys[at] == qkeys)
    out = torch.where(found, words[order[at]], torch.zeros((), dtype=torch.int32, device=query.device))
    return out, int(found.sum())


def lookup_case(ctx, pos, mrgb, repeats):
    ctx.recreate_octree(pos, mrgb)
    half = 1 << ctx.scene_depth
    own = torch.as_tensor(np.ascontiguousarray(pos, np.int16), device=DEV)
    rnd = torch.as_tensor(np.random.default_rng(1).integers(-half, half, (RANDOM, 3)).astype(np.int16), device=DEV)
    case = {"voxels": int(len(pos)), "depth": int(ctx.scene_depth)}
    for name, query, offset in (("own", own, (0, 0, 0)), ("shifted", own, (1, 0, 0)), ("random", rnd, (0, 0, 0))):
        lookup, (leaf, present) = timed(lambda: ctx.lookup_voxels(query, offset), repeats)
        count, counted = timed(lambda: ctx.count_present(query, offset), repeats)
        route, (r_leaf, r_present) = timed(lambda: torch_lookup(ctx, query, offset), repeats)
        assert torch.equal(leaf, r_leaf) and present == counted == r_present, "the two routes disagree"
        case[name] = {"entries": int(len(query)), "present": present, "lookup": lookup, "count": count, "torch_route": route,
                      "lookup_over_route": lookup["median_ms"] / route["median_ms"], "count_over_route": count["median_ms"] / route["median_ms"]}
    return case


def ray_case(ctx, pos, mrgb, size, repeats):
    ctx.recreate_octree(pos, mrgb)
    ctx.camera = Camera(*scenes.bench_camera(size))
    ys, xs = np.divmod(np.arange(SIDE * SIDE), SIDE)
    o, d = ctx.pixel_rays(xs, ys)
    d_o, d_d = torch.as_tensor(o, device=DEV), torch.as_tensor(d, device=DEV)
    free, got = timed(lambda: ctx.pick_device(d_o, d_d), repeats)
    bounded, short = timed(lambda: ctx.pick_device(d_o, d_d, 4.0), repeats)
    host, want = timed(lambda: ctx.pick(o, d), repeats)
    rec = np.zeros(len(o), PICK_HIT_DTYPE)
    for k in rec.dtype.names:
        rec[k] = want[k]
    raw = torch.stack([got["status"].view(torch.int32), got["time"].view(torch.int32)] + [got["normal"].view(torch.int32)[:, i] for i in range(3)]
                      + [got["voxel"][:, i] for i in range(3)] + [got["leaf"]], dim=1).cpu().numpy()
    assert raw.tobytes() == rec.tobytes(), "pick_device and pick disagree"
    return {"rays": int(len(o)), "hits": int((rec["status"] != 0).sum()), "hits_within_4": int((short["status"].view(torch.int32) != 0).sum()),
            "pick_device": free, "pick_device_max_time_4": bounded, "pick": host,
            "pick_device_over_pick": free["median_ms"] / host["median_ms"], "bounded_over_pick": bounded["median_ms"] / host["median_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out")
    args = ap.parse_args()
    result = {"lookup": {}, "rays": {}}
    with Context(SIDE, SIDE) as ctx:
        for name in ("menger", "monu10"):
            pos, mrgb, size = scenes.load_scene(name)
            pos, mrgb = np.ascontiguousarray(pos, np.int16), np.ascontiguousarray(mrgb, np.uint8)
            result["lookup"][name + ".vox"] = lookup_case(ctx, pos, mrgb, args.repeats)
            print(json.dumps({name: result["lookup"][name + ".vox"]}), file=sys.stderr, flush=True)
            result["rays"][name + ".vox"] = ray_case(ctx, pos, mrgb, size, args.repeats)
            print(json.dumps({name: result["rays"][name + ".vox"]}), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
