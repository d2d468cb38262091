"""Host time per trace launch at a frame so small (64 x 64) that the GPU never is the bottleneck: vxrt_render_frames loops in C, one launch
per g frames, and does not wait; the time of the call / launches, 31 blocks of 1000 launches per schedule.  For A/B runs of the host side
of the trace stage (csrc/api_trace.hip): one process per library (VXRT_LIB: scripts/ab_build.sh), the libraries alternating.
usage: python scripts/trace_host_cost.py"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_voxel_raytracer_amd import TRACE, Camera, Context, host, scenes

pos, mrgb, size = scenes.load_scene("3x3x3")
cam = scenes.bench_camera(size)
out = [os.path.basename(host.lib()._name)]
for name, tracer, inflight, g in (("auto 1x1", 0, 1, 1), ("tracer4 1x2", 4, 2, 1), ("auto 16x2", 0, 2, 16)):
    with Context(64, 64, max_bounces=4, tracer=tracer, frames_in_flight=inflight, frames_per_launch=g) as ctx:
        ctx.recreate_octree(pos, mrgb)
        ctx.camera = Camera(*cam)
        ctx.render_frames(TRACE, 200 * g)
        ctx.sync()
        per = []
        for _ in range(31):
            n = 1000
            t0 = time.perf_counter()
            ctx.render_frames(TRACE, n * g)
            t1 = time.perf_counter()
            ctx.sync()
            per.append((t1 - t0) / n * 1e6)
        per.sort()
        out.append(f"{name}: min {per[0]:.2f} q1 {per[len(per) // 4]:.2f} median {statistics.median(per):.2f} us/launch")
print(" | ".join(out), flush=True)
