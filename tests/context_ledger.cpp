// The context's GPU resources, followed through a ledger on the CPU: the real api_context / api_halo / api_extract / api_trace /
// api_scene / api_frame (csrc) linked against stubs of every kernel launcher and of every HIP call they reach (the executable's own
// definitions take precedence over the runtime's, as in scripts/trace_frames_host_stub.cpp).  No GPU is touched.
//   every hipMalloc / hipHostMalloc returns a distinct address backed by host memory, every event and stream a distinct handle;
//   the ledger holds each live handle by kind; releasing one that is not live (or with the wrong call) aborts with a message;
//   hipMemcpy / hipMemset work on the host backing.
// Scenario 1: the whole lifecycle of a context, for several configurations: the ledger must be empty after vxrt_destroy.
// Scenario 2: the same with the Nth allocation / event / stream creation failing, for every N: the entry point that saw the failure
// returns non-zero, a failed vxrt_create leaves *out null, has_scene implies the scene's arrays, vxrt_destroy succeeds, and the
// ledger is empty.  Prints one line per finding; exit status 1 when there is one.
// Build (S = csrc, F = -std=c++17 -O1 --offload-arch=gfx950 --cuda-host-only):
//   hipcc $F -x hip -I$S -Iinclude tests/context_ledger.cpp $S/api_{context,halo,extract,trace,scene,frame}.hip $S/{scene_host,vox_scene,api_host,scene_procedural}.cpp -o ledger
#include <cstdarg>
#include <cstdio>
#include <functional>
#include <map>

#include "ctx.h"
#include "extract.h"
#include "vxrt_extract.h"

namespace {
enum Kind { kDevice, kPinned, kEvent, kStream };
const char* const kKindName[] = {"device buffer", "pinned buffer", "event", "stream"};
std::map<void*, Kind> g_live;
long g_fallible = 0, g_fail_at = 0;   // fallible calls so far in this lifecycle; the one that fails (0: none)
bool g_fired = false;
hipError_t g_last = hipSuccess;
int g_findings = 0;

void finding(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    printf("FINDING: ");
    vprintf(fmt, ap);
    printf("\n");
    va_end(ap);
    g_findings++;
}
hipError_t made(void** out, Kind kind, size_t bytes, hipError_t injected) {
    if (++g_fallible == g_fail_at) { g_fired = true; g_last = injected; return injected; }
    void* p = calloc(bytes ? bytes : 1, 1);
    if (!p) { fprintf(stderr, "ledger: out of host memory\n"); abort(); }
    g_live[p] = kind;
    *out = p;
    return hipSuccess;
}
hipError_t gone(void* p, Kind kind, const char* call) {
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kind) {
        fprintf(stderr, "ledger: %s(%p): %s\n", call, p, it == g_live.end() ? "not live (double free?)" : kKindName[it->second]);
        abort();
    }
    g_live.erase(it);
    free(p);
    return hipSuccess;
}
constexpr size_t kTouch = size_t(1) << 20;   // larger fills are skipped: the backing is zeroed when made, and nothing here reads it
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t n) { return made(p, kDevice, n, hipErrorOutOfMemory); }
hipError_t hipHostMalloc(void** p, size_t n, unsigned) { return made(p, kPinned, n, hipErrorOutOfMemory); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return made(reinterpret_cast<void**>(e), kEvent, 1, hipErrorInvalidValue); }
hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) { return made(reinterpret_cast<void**>(s), kStream, 1, hipErrorInvalidValue); }
hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) { return made(reinterpret_cast<void**>(s), kStream, 1, hipErrorInvalidValue); }
hipError_t hipFree(void* p) { return p ? gone(p, kDevice, "hipFree") : hipSuccess; }
hipError_t hipHostFree(void* p) { return p ? gone(p, kPinned, "hipHostFree") : hipSuccess; }
hipError_t hipEventDestroy(hipEvent_t e) { return gone(e, kEvent, "hipEventDestroy"); }
hipError_t hipStreamDestroy(hipStream_t s) { return gone(s, kStream, "hipStreamDestroy"); }
hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) { memcpy(d, s, n); return hipSuccess; }
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) { if (n <= kTouch) memset(d, v, n); return hipSuccess; }
hipError_t hipGetLastError(void) { const hipError_t e = g_last; g_last = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : (e == hipErrorOutOfMemory ? "out of memory" : "invalid argument"); }
hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int) { *v = 256; return hipSuccess; }
hipError_t hipDeviceGetStreamPriorityRange(int* least, int* greatest) { *least = 0; *greatest = -1; return hipSuccess; }
hipError_t hipEventRecord(hipEvent_t, hipStream_t) { return hipSuccess; }
hipError_t hipEventQuery(hipEvent_t) { return hipSuccess; }
hipError_t hipEventSynchronize(hipEvent_t) { return hipSuccess; }
hipError_t hipEventElapsedTime(float* ms, hipEvent_t, hipEvent_t) { *ms = 0.0f; return hipSuccess; }
hipError_t hipStreamQuery(hipStream_t) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t, unsigned) { return hipSuccess; }
hipError_t hipMemGetAddressRange(hipDeviceptr_t*, size_t*, hipDeviceptr_t) { return hipErrorInvalidValue; }
hipError_t hipPointerGetAttributes(hipPointerAttribute_t*, const void*) { return hipErrorInvalidValue; }
}

namespace vxrt {   // the kernel launchers: nothing runs
hipError_t launch_trace(const TraceArgs&, bool, bool, hipStream_t, unsigned, unsigned) { return hipSuccess; }
hipError_t launch_bounces(const TraceArgs&, bool, const PathQueue*, unsigned**, unsigned* launches, int, unsigned, int, hipStream_t) { *launches += 1; return hipSuccess; }
hipError_t launch_first_hit(const TraceArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_tile_order(uint32_t*, uint32_t*, uint32_t*, uint32_t*, unsigned, unsigned, unsigned, int, hipStream_t) { return hipSuccess; }
hipError_t launch_temporal(const TemporalArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_denoise(const DenoiseArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_spp_accumulate(const SppArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_display_encode(const float4*, uint32_t*, size_t, bool, hipStream_t) { return hipSuccess; }
hipError_t launch_halo_pack(const HaloPackArgs&, hipStream_t) { return hipSuccess; }
hipError_t launch_halo_unpack(float4*, const float4*, const float4*, size_t, hipStream_t) { return hipSuccess; }
hipError_t launch_noise_fill(float*, uint32_t, size_t, hipStream_t) { return hipSuccess; }
hipError_t launch_extract_count(const ExtractLevel&, hipStream_t) { return hipSuccess; }
hipError_t launch_extract_expand(const ExtractLevel&, hipStream_t) { return hipSuccess; }
int scan_total(uint64_t*, uint32_t, hipStream_t, uint64_t* total) { *total = 0; return VXRT_OK; }
unsigned trace_tile_count(int w, int h) { return unsigned((w + 15) / 16) * unsigned((h + 15) / 16); }
void trace_tile_dims(int* w, int* h) { *w = 16; *h = 16; }
bool menger_device_build_supported(uint32_t, uint32_t) { return false; }
int build_menger_svo_device(uint32_t, uint32_t, const uint8_t*, uint32_t, hipStream_t, SvoRecord**, size_t*, int32_t**, size_t*, uint32_t*, SvoRecord*) { return VXRT_E_INVALID; }
int reorder_bottom_treelets(const SvoRecord*, size_t, const std::vector<size_t>&, uint32_t, int, hipStream_t, DeviceBuf<SvoRecord>*) { return VXRT_E_INVALID; }
}  // namespace vxrt

namespace {
struct Cell { uint32_t tracer, inflight, batch, bounces; };

// One context from vxrt_create to vxrt_destroy with fallible call `fail_at` failing (0: none).  Returns the fallible calls it made.
long lifecycle(const Cell& k, long fail_at) {
    char tag[96];
    snprintf(tag, sizeof tag, "tracer %u, %u in flight, %u per launch, %u bounces, failing call %ld", k.tracer, k.inflight, k.batch, k.bounces, fail_at);
    g_fallible = 0; g_fail_at = fail_at; g_fired = false; g_last = hipSuccess;
    static const int16_t pos_a[5][3] = {{0, 0, 0}, {1, 2, 3}, {-8, -8, -8}, {7, 7, 7}, {-3, 4, -5}}, pos_b[3][3] = {{2, 2, 2}, {-1, -1, -1}, {5, -6, 7}};
    static const uint8_t mrgb[5][4] = {{1, 200, 10, 10}, {1, 10, 200, 10}, {2, 10, 10, 200}, {1, 90, 90, 90}, {3, 250, 250, 250}};
    std::vector<float> host(size_t(80) * 48 * 4);
    vxrt_ctx* c = nullptr;
    auto read_both = [&](uint32_t w, uint32_t h) {
        if (int rc = vxrt_read_async(c, VXRT_DENOISED, host.data(), size_t(w) * h * 16, 0)) return rc;
        if (int rc = vxrt_read_async(c, VXRT_DISPLAY_RGBA8_SRGB, host.data(), size_t(w) * h * 4, 1)) return rc;
        if (int rc = vxrt_read_wait(c, 0)) return rc;
        return vxrt_read_wait(c, 1);
    };
    const std::pair<const char*, std::function<int()>> steps[] = {
        {"vxrt_create", [&] {
             vxrt_config cfg{};
             cfg.width = 64; cfg.height = 48; cfg.max_bounces = k.bounces; cfg.tracer = k.tracer; cfg.frames_in_flight = k.inflight; cfg.frames_per_launch = k.batch;
             const int rc = vxrt_create(&cfg, &c);
             if (rc != VXRT_OK && c != nullptr) { finding("%s: a failed vxrt_create left *out non-null", tag); c = nullptr; }
             return rc;
         }},
        {"vxrt_set_voxels", [&] { return vxrt_set_voxels(c, pos_a, mrgb, 5); }},
        {"vxrt_set_voxels (second)", [&] { return vxrt_set_voxels(c, pos_b, mrgb, 3); }},
        {"vxrt_render_frames", [&] { return vxrt_render_frames(c, VXRT_ALL, 2); }},
        {"vxrt_get_voxels", [&] { size_t n = 0; return vxrt_get_voxels(c, nullptr, nullptr, nullptr, nullptr, 0, &n); }},
        {"vxrt_read_async", [&] { return read_both(64, 48); }},
        {"vxrt_resize", [&] { return vxrt_resize(c, 80, 32); }},
        {"tail capacity, larger", [&] { return vxrt_set_option(c, VXRT_OPT_TAIL_CAPACITY, 1u << 20); }},
        {"tail capacity, smaller", [&] { return vxrt_set_option(c, VXRT_OPT_TAIL_CAPACITY, 64); }},
        {"tail capacity, larger again", [&] { return vxrt_set_option(c, VXRT_OPT_TAIL_CAPACITY, 128); }},
        {"vxrt_read_async after the resize", [&] { return read_both(80, 32); }},
        {"vxrt_device_image", [&] { void* p = nullptr; size_t n = 0; return vxrt_device_image(c, VXRT_DISPLAY_BGRA8_SRGB, &p, &n); }},
        {"vxrt_render_spp", [&] { return vxrt_render_spp(c, VXRT_ALL, 3); }},
        {"vxrt_resize back", [&] { return vxrt_resize(c, 64, 48); }},
        {"vxrt_read_async, a larger stage", [&] { return read_both(64, 48); }},
    };
    for (const auto& [name, step] : steps) {
        const bool fired_before = g_fired;
        const int rc = step();
        if (g_fired && !fired_before && rc == VXRT_OK) finding("%s: %s returned VXRT_OK although its HIP call failed", tag, name);
        if (rc != VXRT_OK && !g_fired) finding("%s: %s failed with nothing injected: %s", tag, name, vxrt_last_error());
        if (rc != VXRT_OK || g_fired) break;
    }
    if (c != nullptr) {
        if (c->has_scene && (c->d_svo == nullptr || c->d_leaves == nullptr)) finding("%s: has_scene with null scene arrays", tag);
        if (vxrt_destroy(c) != VXRT_OK) finding("%s: vxrt_destroy failed: %s", tag, vxrt_last_error());
    }
    if (!g_live.empty()) {
        size_t n[4] = {0, 0, 0, 0};
        for (const auto& e : g_live) { n[e.second]++; free(e.first); }
        g_live.clear();
        finding("%s: leaked %zu device buffers, %zu pinned buffers, %zu events, %zu streams", tag, n[0], n[1], n[2], n[3]);
    }
    if (fail_at != 0 && !g_fired) finding("%s: the call to fail was never reached", tag);
    return g_fallible;
}
}  // namespace

int main() {
    std::vector<Cell> cells;
    for (uint32_t tracer : {1u, 4u})
        for (uint32_t inflight : {1u, 2u})
            for (uint32_t batch : {1u, 8u}) cells.push_back(Cell{tracer, inflight, batch, 4});
    cells.push_back(Cell{4, 2, 8, 6});   // from 6 bounces on the tail compacts again: two queues per stream
    long lifecycles = 0, injected = 0;
    for (const Cell& k : cells) {
        const long fallible = lifecycle(k, 0);
        lifecycles++;
        for (long n = 1; n <= fallible; n++, injected++) lifecycle(k, n);
    }
    if (g_findings != 0) { printf("%d findings\n", g_findings); return 1; }
    printf("ok %ld lifecycles, %ld injected failures\n", lifecycles, injected);
    return 0;
}
