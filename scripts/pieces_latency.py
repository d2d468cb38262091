"""Latency of the component table and of the detached pieces on the device (vxrt_component_table_device, vxrt_detached_pieces_device,
include/vxrt_pieces.h), read against the route the project offered before them, on the same machine in the same run:
label_components (or detached_voxels) and then torch.unique plus scatter_reduce (amin, amax, sum) on the device, per statistic.
Prints one JSON document (profiles/pieces/).

Cases: the voxel lists of menger.vox and monu10.vox (tests/golden/scenes/) and a 128^3 random grid at occupancy 0.31, each at
connectivity 6 and 26 with the list already on the device: `label` (one vxrt_label_components_device call), `table` (one
vxrt_component_table_device call writing label, id and info), `table_wrapper` (Context.component_table: a count call and a fetch
call) and `torch_route`; `overhead_ms` is table minus label, the medians: what the extra reduction costs.  detached_pieces of
menger.vox and monu10.vox loaded as scenes with one y layer cleared, the anchor box their lowest y layer: `count` (the count-only C
call), `fetch` (the wrapper: count, then fetch) and `torch_route` (detached_voxels, then the same chain).  Host clock around the
synchronous call, after one warm-up, median / min / max over the repeats.  The script also asserts that both routes agree.
  --grid N          side of the random grid (default 128)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_voxel_raytracer_amd import Context, scenes  # noqa: E402
from voxelize_latency import DEV, stats_ms, sync_timed  # noqa: E402

CONNECTIVITIES = (6, 26)


def torch_table(pos, label):
    """the parent's route from a labelling to (id, first, voxels, min, max, sum): torch.unique and scatter_reduce on the device"""
    lab = label.view(torch.int32).to(torch.int64)
    first, ids = torch.unique(lab, return_inverse=True)            # ascending labels: the numbering
    k = len(first)
    u = pos.to(torch.int64) + 32768
    cell, where = torch.unique((u[:, 0] << 32) | (u[:, 1] << 16) | u[:, 2], return_inverse=True)      # the distinct positions
    cid = torch.empty(len(cell), dtype=torch.int64, device=pos.device).scatter_(0, where, ids)
    p = torch.stack([cell >> 32, (cell >> 16) & 0xFFFF, cell & 0xFFFF], dim=1) - 32768
    index = cid[:, None].expand(-1, 3)
    voxels = torch.bincount(cid, minlength=k)
    lo = torch.full((k, 3), 1 << 20, dtype=torch.int64, device=pos.device).scatter_reduce(0, index, p, "amin")
    hi = torch.full((k, 3), -(1 << 20), dtype=torch.int64, device=pos.device).scatter_reduce(0, index, p, "amax")
    total = torch.zeros((k, 3), dtype=torch.int64, device=pos.device).scatter_reduce(0, index, p, "sum")
    return ids, first, voxels, lo, hi, total


def same_table(table, ids, route):
    r_ids, first, voxels, lo, hi, total = route
    return (torch.equal(ids.view(torch.int32).to(torch.int64), r_ids) and torch.equal(table["first"].view(torch.int32).to(torch.int64), first)
            and torch.equal(table["voxels"].view(torch.int32).to(torch.int64), voxels) and torch.equal(table["min"].to(torch.int64), lo)
            and torch.equal(table["max"].to(torch.int64), hi) and torch.equal(table["sum"], total))


def timed(fn, repeats):
    samples, out = [], None
    for r in range(repeats + 1):
        dt, out = sync_timed(fn)
        if r:
            samples.append(dt)
    return stats_ms(samples), out


def table_case(ctx, pos, repeats):
    L = ctx._L
    d_pos = torch.as_tensor(np.ascontiguousarray(pos, np.int16), device=DEV)
    n = len(pos)
    out_label, out_ids = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    got = C.c_size_t(0)
    case = {"entries": int(n)}
    for conn in CONNECTIVITIES:
        head = (ctx._h, C.c_void_p(d_pos.data_ptr()), C.c_size_t(n), C.c_uint32(conn))
        label, rc = timed(lambda: L.vxrt_label_components_device(*head, C.c_void_p(out_label.data_ptr()), C.byref(got)), repeats)
        assert rc == 0, (L.vxrt_last_error() or b"").decode()
        k = int(got.value)
        info = torch.empty(k * ctx.PIECE_BYTES, dtype=torch.uint8, device=DEV)
        table, rc = timed(lambda: L.vxrt_component_table_device(*head, C.c_void_p(out_label.data_ptr()), C.c_void_p(out_ids.data_ptr()),
                                                                C.c_void_p(info.data_ptr()), C.c_size_t(k), C.byref(got)), repeats)
        assert rc == 0 and got.value == k, (L.vxrt_last_error() or b"").decode()
        wrapper, (_, ids, tab) = timed(lambda: ctx.component_table(d_pos, conn), repeats)
        route, out = timed(lambda: torch_table(d_pos, ctx.label_components(d_pos, conn)[0]), repeats)
        assert same_table(tab, ids, out) and torch.equal(out_ids, ids.view(torch.int32)), "the two routes disagree"
        case[f"connectivity {conn}"] = {"components": k, "label": label, "table": table, "table_wrapper": wrapper, "torch_route": route,
                                        "overhead_ms": table["median_ms"] - label["median_ms"]}
    return case


def scene_case(ctx, pos, mrgb, repeats):
    L = ctx._L
    lo, hi = pos.min(axis=0).astype(int), pos.max(axis=0).astype(int)
    layer = int(lo[1]) + (int(hi[1]) - int(lo[1])) // 3
    keep = pos[:, 1] != layer
    ctx.recreate_octree(pos[keep], mrgb[keep])
    anchor = (tuple(lo.tolist()), (int(hi[0]) + 1, int(lo[1]) + 1, int(hi[2]) + 1))
    box = [(C.c_int32 * 3)(*a) for a in anchor]
    got, pieces = C.c_size_t(0), C.c_size_t(0)
    case = {"voxels": int(keep.sum())}
    for conn in CONNECTIVITIES:
        count, rc = timed(lambda: L.vxrt_detached_pieces_device(ctx._h, box[0], box[1], C.c_uint32(conn), C.c_uint32(0), C.c_uint32(0xFFFFFFFF),
                                                                None, None, None, C.c_size_t(0), C.byref(got), None, C.c_size_t(0), C.byref(pieces)),
                          repeats)
        assert rc == 0, (L.vxrt_last_error() or b"").decode()
        fetch, (d_pos, _, piece, tab) = timed(lambda: ctx.detached_pieces(*anchor, connectivity=conn), repeats)

        def parent_route():
            p, _ = ctx.detached_voxels(*anchor, connectivity=conn)
            return torch_table(p, ctx.label_components(p, conn)[0]) if len(p) else None
        route, out = timed(parent_route, repeats)
        assert out is None or same_table(tab, piece, out), "the two routes disagree"
        case[f"connectivity {conn}"] = {"detached": int(got.value), "pieces": int(pieces.value), "count": count, "fetch": fetch, "torch_route": route}
    return case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--out")
    args = ap.parse_args()
    result = {"component_table": {}, "detached_pieces": {}}
    with Context(64, 64) as ctx:
        lists = {name + ".vox": scenes.load_scene(name)[:2] for name in ("menger", "monu10")}
        grid = np.argwhere(np.random.default_rng(1).random((args.grid,) * 3) < 0.31) - args.grid // 2
        for name, pos in list((n, l[0]) for n, l in lists.items()) + [(f"random {args.grid}^3 at 0.31", grid)]:
            result["component_table"][name] = table_case(ctx, pos, args.repeats)
            print(json.dumps({name: result["component_table"][name]}), file=sys.stderr, flush=True)
        for name, (pos, mrgb) in lists.items():
            result["detached_pieces"][name] = scene_case(ctx, pos, mrgb, args.repeats)
            print(json.dumps({name: result["detached_pieces"][name]}), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
