// Host-only timing of trace_frames (csrc/api_trace.hip): every HIP call and every kernel launcher it reaches is a stub, so what is
// left is the host code of the trace stage's scheduling — nanoseconds per call, measurable without a GPU.  For A/B runs of two versions
// of api_trace.hip (S = the csrc directory of the version; F = the flags of gpu_voxel_raytracer_amd/_build.py without -shared -fPIC):
//   hipcc $F -x hip -I$S -c $S/api_trace.hip -o api.o && hipcc $F -x hip -I$S -c scripts/trace_frames_host_stub.cpp -o stub.o
//   hipcc --offload-arch=gfx950 api.o stub.o -o stub && taskset -c 3 ./stub TRACER INFLIGHT FRAMES_PER_LAUNCH     (0 1 1 = the latency case)
// The stubs of launch_trace copy the arguments as the real one does; the stub call total printed must be equal for both versions.
#include <chrono>
#include <cstdio>
#include <algorithm>
#include "ctx.h"
static volatile unsigned long long g_calls = 0;
#define STUB { g_calls = g_calls + 1; return hipSuccess; }
extern "C" {
hipError_t hipEventRecord(hipEvent_t, hipStream_t) STUB
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) STUB
hipError_t hipEventQuery(hipEvent_t) STUB
hipError_t hipEventSynchronize(hipEvent_t) STUB
hipError_t hipMemcpyAsync(void*, const void*, size_t, hipMemcpyKind, hipStream_t) STUB
hipError_t hipMemsetAsync(void*, int, size_t, hipStream_t) STUB
// what the set-up below allocates through the context's owners (not counted: trace_frames allocates nothing)
hipError_t hipMalloc(void** p, size_t n) { *p = calloc(n, 1); return hipSuccess; }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { *p = calloc(n, 1); return hipSuccess; }
hipError_t hipFree(void* p) { free(p); return hipSuccess; }
hipError_t hipHostFree(void* p) { free(p); return hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t) { return hipSuccess; }
hipError_t hipStreamDestroy(hipStream_t) { return hipSuccess; }
}
namespace vxrt {
hipError_t launch_trace(const TraceArgs& a, bool, bool, hipStream_t, unsigned, unsigned) { TraceArgs b = a; g_calls = g_calls + b.batch; return hipSuccess; }   // the real one copies the arguments too
hipError_t launch_bounces(const TraceArgs&, bool, const PathQueue*, unsigned**, unsigned* l, int, unsigned, int, hipStream_t) { *l += 1; STUB }
hipError_t launch_first_hit(const TraceArgs&, hipStream_t) STUB
hipError_t launch_walk_list(const uint32_t*, const uint32_t*, uint32_t*, uint32_t*, uint32_t*, unsigned, hipStream_t) STUB
hipError_t launch_tile_order(uint32_t*, uint32_t*, uint32_t*, uint32_t*, unsigned, unsigned, unsigned, int, hipStream_t) STUB
unsigned trace_tile_count(int w, int h) { return unsigned((w + 7) / 8) * unsigned((h + 7) / 8); }
void trace_tile_dims(int* w, int* h) { *w = 8; *h = 8; }
CameraBasis camera_axis_scaled(const float d[3], float, uint32_t, uint32_t) { CameraBasis b{}; b.right[0] = 1; b.up[1] = 1; for (int i = 0; i < 3; i++) b.forward_ray[i] = d[i]; return b; }
int sync_all(vxrt_ctx*) { return 0; }
bool use_wide(const vxrt_ctx* c) { return c->d_wide != nullptr && c->scene_format == 1; }
void set_error(const std::string&) {}
EventPair take_pair(vxrt_ctx*, int) { return EventPair{}; }
}
int main(int argc, char** argv) {
    const int tracer = atoi(argv[1]), inflight = atoi(argv[2]); const uint32_t g = uint32_t(atoi(argv[3]));
    static vxrt_ctx c;
    c.cfg.width = 64; c.cfg.height = 64; c.cfg.max_bounces = 4;
    c.band.width = 64; c.band.local_rows = 64;
    c.inflight = inflight; c.batch = int(g);
    c.trace_variant = tracer == 0 ? 4 : (tracer == 1 ? 0 : tracer); c.auto_tracer = tracer == 0;
    c.trace_streams.assign(size_t(inflight), nullptr);
    c.ring.resize(size_t(inflight) * g + 2);
    c.schedules.resize(size_t(inflight)); c.launch_events.resize(size_t(inflight) * 2); c.launch_event_turn.assign(size_t(inflight), 0u);
    if (c.trace_variant) { c.queues.resize(size_t(inflight)); for (int i = 0; i < inflight; i++) { (void)c.queues[i].counts3.alloc(3 * 64 * 16); (void)c.queues[i].host_counts.alloc(64 * 16); (void)c.queues[i].hitq[0].alloc(64); } }
    if (g >= 2) { c.first_hits.resize(size_t(inflight)); for (auto& fh : c.first_hits) (void)fh.alloc(4); c.first_hit_walked.resize(size_t(inflight)); c.first_hit_readers.assign(size_t(inflight) * size_t(inflight), nullptr); }
    c.shard_capacity = 64; c.shard_capacity_max = 64; c.svo_count = 1000; c.leaf_count = 1000; c.depth = 5;
    c.uniforms.sun_size = 0.05f; c.uniforms.sun_strength = 1; c.box_valid = true;
    int slots[32]; Cam cams[32], olds[32];
    double best[7];
    for (int rep = 0; rep < 7; rep++) {
        const int n = 2000000 / int(g > 4 ? 4 : 1);
        auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < n; i++) if (trace_frames(&c, g, false, slots, cams, olds)) return 1;
        best[rep] = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / n;
    }
    std::sort(best, best + 7);
    printf("tracer %d %ux%d: min %.1f median %.1f ns per trace_frames (%llu stub calls)\n", tracer, g, inflight, best[0], best[3], (unsigned long long)g_calls);
}
