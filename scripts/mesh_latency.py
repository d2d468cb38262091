"""Latency of vxrt_mesh_voxels_device (include/vxrt_mesh.h), read against the route a host had before it, on the same machine in
the same run.  Prints one JSON document (profiles/mesh/).

Lists, already on the device: a solid icosphere of radius `--radius` from Context.voxelize_solid, its MORPH_SURFACE shell (one
step, connectivity 6), and a flat slab of `--slab` x `--slab` x 2 voxels in three colours.  Per list:
  `faces`, `runs`   Context.mesh_voxels in each mode with cap=None: the counting call and the emitting call
  `runs_one_call`   MESH_RUNS with cap=(8 n, 12 n), the a-priori bounds: one call
  `host`            the list copied to the host and meshed there with numpy, unmerged faces only (the rule of the header, vectorised:
                    sorted keys, one searchsorted per direction, the corners through unique); the copy is inside the clock
The script asserts that the host route and MESH_FACES give the same vertices, triangles and bytes.
`--device-only` leaves the host route out: the run under `rocprofv3 --kernel-trace --stats` that splits a call's time by kernel.
Host clock around the synchronous call, after one warm-up, median / min / max over the repeats."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpu_voxel_raytracer_amd import Context  # noqa: E402
from gpu_voxel_raytracer_amd.host import MESH_FACES, MESH_RUNS, MORPH_SURFACE  # noqa: E402
from pieces_latency import timed  # noqa: E402
from voxelize_latency import DEV, icosphere  # noqa: E402

DIRECTIONS = ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (0, 1, 0), (1, 0, 0))


def host_faces(pos, mrgb):
    """The header's rule in FACES mode on the host -> (verts float32 [V,3], tris uint32 [T,3], tri_mrgb uint8 [T,4]).  pos and mrgb
    are device tensors: the copy is part of the route."""
    p = pos.cpu().numpy().astype(np.int64) + 32768
    b = mrgb.cpu().numpy().copy()
    b[:, 0] &= 0x7F
    lin = (p[:, 0] << 32) | (p[:, 1] << 16) | p[:, 2]
    order = np.argsort(lin, kind="stable")
    last = np.ones(len(lin), bool)
    last[:-1] = lin[order][1:] != lin[order][:-1]          # the last entry of a position wins
    order = order[last]
    p, b, lin = p[order], b[order], lin[order]
    keys, words, quads = [], [], []
    for d, o in enumerate(DIRECTIONS):
        q = p + np.array(o)
        inside = ((q >= 0) & (q <= 65535)).all(axis=1)
        qlin = (q[:, 0] << 32) | (q[:, 1] << 16) | q[:, 2]
        at = np.minimum(np.searchsorted(lin, qlin), len(lin) - 1)
        bare = ~(inside & (lin[at] == qlin))
        a = next(i for i in range(3) if o[i])
        f = p[bare]
        w, fb, fc = f[:, a] + (1 if o[a] > 0 else 0), f[:, (a + 1) % 3], f[:, (a + 2) % 3]
        keys.append((d << 49) | (w << 32) | (fb << 16) | fc)
        words.append(b[bare])
        corners = np.zeros((len(f), 4, 3), np.int64)
        bs = (fb, fb + 1, fb + 1, fb) if o[a] > 0 else (fb, fb, fb + 1, fb + 1)
        cs = (fc, fc, fc + 1, fc + 1) if o[a] > 0 else (fc, fc + 1, fc + 1, fc)
        for i in range(4):
            corners[:, i, a], corners[:, i, (a + 1) % 3], corners[:, i, (a + 2) % 3] = w, bs[i], cs[i]
        quads.append(corners)
    keys, words, quads = np.concatenate(keys), np.concatenate(words), np.concatenate(quads)
    order = np.argsort(keys, kind="stable")
    words, quads = words[order], quads[order]
    ckeys = (quads[:, :, 0] << 34) | (quads[:, :, 1] << 17) | quads[:, :, 2]
    uniq, index = np.unique(ckeys.reshape(-1), return_inverse=True)
    index = index.reshape(-1, 4)
    verts = np.stack([uniq >> 34, (uniq >> 17) & 0x1FFFF, uniq & 0x1FFFF], -1) - 32768
    tris = np.stack([index[:, [0, 1, 2]], index[:, [0, 2, 3]]], 1).reshape(-1, 3)
    return verts.astype(np.float32), tris.astype(np.uint32), np.repeat(words, 2, axis=0)


def case(ctx, pos, mrgb, repeats, device_only):
    n = len(pos)
    out = {"entries": int(n)}
    out["faces"], (f_verts, f_tris, f_mrgb) = timed(lambda: ctx.mesh_voxels(pos, mrgb, MESH_FACES), repeats)
    out["runs"], (r_verts, r_tris, _) = timed(lambda: ctx.mesh_voxels(pos, mrgb, MESH_RUNS), repeats)
    out["runs_one_call"], (o_verts, o_tris, _) = timed(lambda: ctx.mesh_voxels(pos, mrgb, MESH_RUNS, cap=(8 * n, 12 * n)), repeats)
    assert torch.equal(o_verts, r_verts) and torch.equal(o_tris, r_tris), "counting first and the one call disagree"
    out["faces_mesh"] = {"vertices": int(len(f_verts)), "triangles": int(len(f_tris))}
    out["runs_mesh"] = {"vertices": int(len(r_verts)), "triangles": int(len(r_tris))}
    if not device_only:
        out["host"], (h_verts, h_tris, h_mrgb) = timed(lambda: host_faces(pos, mrgb), repeats)
        assert np.array_equal(f_verts.cpu().numpy(), h_verts) and np.array_equal(f_tris.cpu().numpy().view(np.uint32), h_tris), "the two routes disagree"
        assert np.array_equal(f_mrgb.cpu().numpy(), h_mrgb), "the two routes' bytes disagree"
        out["faces_over_host"] = out["faces"]["median_ms"] / out["host"]["median_ms"]
        out["runs_over_host"] = out["runs"]["median_ms"] / out["host"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--radius", type=float, default=60.0)
    ap.add_argument("--slab", type=int, default=512)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    rng = np.random.default_rng(7)
    result = {}
    with Context(64, 64) as ctx:
        verts, tris = icosphere(4, args.radius)
        solid = ctx.voxelize_solid(verts, tris, None, (1, 200, 120, 40), interior_only=True)
        shell = ctx.morph_voxels(*solid, MORPH_SURFACE, 6, 1)
        g = np.arange(args.slab) - args.slab // 2
        cells = np.stack(np.meshgrid(g, g, [0, 1], indexing="ij"), -1).reshape(-1, 3).astype(np.int16)
        palette = np.array([[1, 200, 10, 10], [2, 10, 200, 10], [3, 10, 10, 200]], np.uint8)
        slab = (torch.as_tensor(cells, device=DEV), torch.as_tensor(palette[rng.integers(0, 3, len(cells))], device=DEV))
        lists = {f"solid icosphere, radius {args.radius:g}": solid, "its surface shell": shell, f"slab {args.slab} x {args.slab} x 2, three colours": slab}
        for name, (pos, mrgb) in lists.items():
            result[name] = case(ctx, pos.contiguous(), mrgb.contiguous(), args.repeats, args.device_only)
            print(json.dumps({name: result[name]}), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()
