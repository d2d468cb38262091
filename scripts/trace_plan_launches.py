"""Which kernels a trace launch goes out as, configuration by configuration: the run to put under `rocprofv3 --kernel-trace --stats` once
per library (VXRT_LIB selects it: scripts/ab_build.sh) when the host side of the trace stage (csrc/api_trace.hip: plan_trace and the
issuing functions) changes and the kernels do not.  Two libraries that schedule alike give the same table of kernel name -> calls.

    python scripts/trace_plan_launches.py --list                   the configurations: index, 1 if it needs a -DVXRT_VARIANTS=1 library, name
    python scripts/trace_plan_launches.py INDEX                    renders configuration INDEX's launches and exits
    python scripts/trace_plan_launches.py --table DIR              kernel name -> calls of the rocprofv3 output below DIR, as JSON
    python scripts/trace_plan_launches.py --compare A.json B.json  "identical" or the kernels whose counts differ; exit status 1 if any

Every render call is followed by a sync, so what the event polls of a launch see does not depend on timing."""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

W, H, LAUNCHES = 256, 144, 4
# name, vxrt_config.tracer (0 auto), frames in flight, frames per launch, bounces, options by name (host.OPT_*), needs the variants library
CONFIGS = [
    ("auto, one frame at a time", 0, 1, 1, 4, {}, False),
    ("auto, 16 frames x 2 in flight, shared primary on", 0, 2, 16, 4, {"SHARED_PRIMARY": 1}, False),
    ("auto, 16 frames x 2 in flight, shared primary off", 0, 2, 16, 4, {"SHARED_PRIMARY": 0}, False),
    ("auto, 6 frames x 1, frame lanes off", 0, 1, 6, 4, {"FRAME_LANES": 0}, False),
    ("tracer 1, raster tile order", 1, 1, 1, 4, {"TILE_ORDER": 0}, False),
    ("tracer 1, 8 frames x 2, shared primary on", 1, 2, 8, 4, {"SHARED_PRIMARY": 1}, False),
    ("tracer 1, 8 frames x 2, shared primary off", 1, 2, 8, 4, {"SHARED_PRIMARY": 0}, False),
    ("tracer 4", 4, 1, 1, 4, {}, False),
    ("tracer 4, tail from hit 2, 4 in flight", 4, 4, 1, 4, {"TAIL_FROM": 2}, False),
    ("tracer 4, 8 bounces: the tail compacts again", 4, 3, 4, 8, {}, False),
    ("tracer 4, tail from the first hit, split 0x6", 4, 3, 1, 4, {"TAIL_FROM": 0, "TAIL_SPLIT": 0x6}, False),
    ("tracer 4, long tiles 100, 2 in flight", 4, 2, 1, 4, {"LONG_TILES": 100}, True),
    ("tracer 4, long tiles 500, 4 frames, shared primary on", 4, 1, 4, 4, {"LONG_TILES": 500, "TILE_SPREAD": 0, "TAIL_CAPACITY": 64}, True),
    ("tracer 4, fused tail", 4, 1, 1, 4, {"FUSED_TAIL": 1}, True),
    ("tracer 4, fused tail, 8 frames x 3, small queues", 4, 3, 8, 4, {"FUSED_TAIL": 1, "TAIL_CAPACITY": 64}, True),
    ("tracer 5", 5, 1, 1, 4, {}, True),
    ("tracer 5, tail from hit 2, 4 frames x 2", 5, 2, 4, 4, {"TAIL_FROM": 2}, True),
    ("wide records, auto", 0, 1, 1, 4, {"SCENE_FORMAT": 1}, True),
    ("wide records, tracer 1, 8 frames", 1, 1, 8, 4, {"SCENE_FORMAT": 1}, True),
    ("wide records, tracer 4, 8 bounces, 3 in flight", 4, 3, 4, 8, {"SCENE_FORMAT": 1, "TAIL_CAPACITY": 128}, True),
    ("priority split, tracer 1, 4 frames", 1, 1, 4, 4, {"TRACE_PRIORITY": 1}, True),
    ("priority split, auto, 8 frames x 2, shared primary on", 0, 2, 8, 4, {"TRACE_PRIORITY": 1, "SHARED_PRIMARY": 1}, True),
    ("priority split, auto, 8 frames x 2, shared primary off", 0, 2, 8, 4, {"TRACE_PRIORITY": 1, "SHARED_PRIMARY": 0}, True),
]


def render(index):
    from gpu_voxel_raytracer_amd import TRACE, Camera, Context, host, scenes
    name, tracer, inflight, g, bounces, options, _ = CONFIGS[index]
    pos, mrgb, size = scenes.load_scene("menger")
    tuning = [(getattr(host, "OPT_" + k), v) for k, v in options.items()]
    with Context(W, H, max_bounces=bounces, tracer=tracer, frames_in_flight=inflight, frames_per_launch=g, tuning=tuning) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = Camera(*scenes.bench_camera(size))
        for _ in range(LAUNCHES * inflight):
            ctx.render_frames(TRACE, g)
            ctx.sync()
        st = ctx.stats()
        print(json.dumps({"config": index, "name": name, "library": os.path.basename(host.lib()._name), "rays": st.rays,
                          "frame_lane_launches": st.frame_lane_launches, "shared_primary_launches": ctx.shared_primary_launches(),
                          "split_launches": st.split_launches}))


def table(directory):
    """kernel name -> calls: from the kernel_stats CSV of --stats, or counted from the kernel_trace CSV."""
    counts = {}
    stats = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    for path in stats:
        for r in csv.DictReader(open(path)):
            counts[r["Name"]] = counts.get(r["Name"], 0) + int(r["Calls"])
    if not stats:
        for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                counts[r["Kernel_Name"]] = counts.get(r["Kernel_Name"], 0) + 1
    if not counts:
        raise SystemExit(f"no kernel statistics below {directory}")
    return dict(sorted(counts.items()))


def compare(a, b):
    ta, tb = json.load(open(a)), json.load(open(b))
    diff = {k: (ta.get(k, 0), tb.get(k, 0)) for k in sorted(set(ta) | set(tb)) if ta.get(k, 0) != tb.get(k, 0)}
    print("identical" if not diff else "DIFFERENT: " + json.dumps(diff), f"({len(ta)} kernels, {sum(ta.values())} calls)")
    return 1 if diff else 0


if __name__ == "__main__":
    if sys.argv[1:2] == ["--list"]:
        for i, cfg in enumerate(CONFIGS):
            print(i, int(cfg[6]), cfg[0])
    elif sys.argv[1:2] == ["--table"]:
        print(json.dumps(table(sys.argv[2]), indent=1))
    elif sys.argv[1:2] == ["--compare"]:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        render(int(sys.argv[1]))
