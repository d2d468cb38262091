// ctx.h — the context behind the C ABI of libvxrt (include/vxrt.h) and the internal helpers its translation units share.
// The ABI is split along its seams:
//   api_context.hip  create / destroy / resize, parameters, options, outputs, statistics     (Context::new, resize, update_bindings)
//   api_scene.hip    scene upload: voxel list -> octree -> device records; procedural scene  (Context::recreate_octree)
//   api_trace.hip    scheduling of the trace stage: frame slots, streams, tile order, tail queues
//   api_frame.hip    frame sequencing: vxrt_render* and the post stages                        (Context::render)
//   api_halo.hip     the multi-rank halo: layout, pack / unpack, interior / edge denoise split
//   api_host.cpp     host-only helpers (no GPU): .vox decoding, octree words, camera basis, noise archive
//   api_debug.hip    test hooks and diagnostics
//   api_edit.hip     in-place scene edits and the pick query (vxrt_edit.h)
//   api_extract.hip  the scene's voxels read back from the device, whole or by box (vxrt_extract.h)
//   api_device_scene.hip  a scene built on the device from a voxel list in device memory (vxrt_device_scene.h)
//   api_scene_depth.hip   the octree depth of a loaded scene changed in place (vxrt_scene_depth.h)
//   api_compact.hip  an edited scene re-laid as a fresh build lies, and the storage counts (vxrt_compact.h)
//   api_query.hip    voxel lookups and bounded ray casts against the scene from device memory (vxrt_query.h)
//   api_transform.hip  a device voxel list resampled under a fixed-point affine map (vxrt_transform.h)
//   api_setops.hip   two device voxel lists combined: union, intersection, difference, delta (vxrt_setops.h)
//   api_morph.hip    a device voxel list dilated, eroded, or cut to its surface layer or margin ring (vxrt_morph.h)
//   api_mesh.hip     a device voxel list's exposed faces as an indexed triangle mesh (vxrt_mesh.h)
//   api_shape.hip    a box, ball, cylinder or capsule rasterised into a device voxel list (vxrt_shape.h)
//   api_distance.hip a device voxel list's exact squared Euclidean distance transform; ball dilate and erode (vxrt_distance.h)
//   list_ops.hip     no entry point: the host pipeline those six share (list_ops.h)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vxrt.h"
#include "../../include/vxrt_debug.h"
#include "../../include/vxrt_host.h"
#include "kernels.h"
#include "owned.h"
#include "scene_host.h"

namespace vxrt {
const std::string& last_error();

constexpr size_t kNoiseCount = size_t(512) * 128 * 128;  // shaders/voxels.comp:65-67

inline int hip_fail(hipError_t e, const char* what) {
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return VXRT_E_DEVICE;
}
// Nothing may unwind across the C boundary: every int-returning entry point is a function-try-block ending in this.
#define VXRT_CATCH                                                                                                         \
    catch (const std::bad_alloc&) { vxrt::set_error("out of host memory"); return VXRT_E_INVALID; }                        \
    catch (const std::exception& e) { vxrt::set_error(std::string("internal error: ") + e.what()); return VXRT_E_INVALID; } \
    catch (...) { vxrt::set_error("internal error"); return VXRT_E_INVALID; }

#define HIP_TRY(expr)                                           \
    do {                                                        \
        hipError_t e_ = (expr);                                 \
        if (e_ != hipSuccess) return vxrt::hip_fail(e_, #expr); \
    } while (0)

// a device allocation of bytes; as a local it lives as long as the entry point that made it (released on every return path)
using ScratchBuffer = DeviceBuf<void>;

// A failed device allocation of an entry point: clears the HIP error, sets "<who>: allocating <what>: <hip error>", VXRT_E_DEVICE.
inline int alloc_failed(hipError_t e, const char* who, const char* what) {
    (void)hipGetLastError();
    set_error(std::string(who) + ": allocating " + what + ": " + hipGetErrorString(e));
    return VXRT_E_DEVICE;
}

// b->alloc(bytes), or alloc_failed.  A request for 0 bytes gets 16, so every buffer is non-null.
inline int alloc_scratch(ScratchBuffer* b, size_t bytes, const char* who, const char* what) {
    const hipError_t e = b->alloc(bytes ? bytes : 16);
    if (e == hipSuccess) return VXRT_OK;
    return alloc_failed(e, who, what);
}

// `count` voxels into a caller's device arrays pos (3 int16 each) and mrgb (4 bytes each) by write(int16_t*, uint32_t*), which
// enqueues the kernel on s: in place where the kernel's stores fit the arrays' alignment (2 bytes per coordinate, 4 per mrgb word);
// otherwise staged (in `stage`, which must outlive the work on s) and copied.  Does not wait.
template <typename Write>
int write_voxels_staged(void* pos, void* mrgb, size_t count, hipStream_t s, const char* who, ScratchBuffer (&stage)[2], Write write) {
    const bool direct = (reinterpret_cast<uintptr_t>(pos) & 1u) == 0u && (reinterpret_cast<uintptr_t>(mrgb) & 3u) == 0u;
    if (direct) {
        HIP_TRY(write(static_cast<int16_t*>(pos), static_cast<uint32_t*>(mrgb)));
        return VXRT_OK;
    }
    if (int rc = alloc_scratch(&stage[0], count * 3 * sizeof(int16_t), who, "the positions")) return rc;
    if (int rc = alloc_scratch(&stage[1], count * 4, who, "the mrgb words")) return rc;
    HIP_TRY(write(stage[0].as<int16_t>(), stage[1].as<uint32_t>()));
    HIP_TRY(hipMemcpyAsync(pos, stage[0].get(), count * 3 * sizeof(int16_t), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(mrgb, stage[1].get(), count * 4, hipMemcpyDeviceToDevice, s));
    return VXRT_OK;
}

struct EventPair {   // handles, not owned: the events live in vxrt_ctx::pair_events
    hipEvent_t a = nullptr, b = nullptr;
    int stage = 0;  // 0 trace, 1 temporal, 2 denoise, 3 halo pack, 4 halo unpack
};

// the sky cull of a launch as the kernels get it (TraceArgs::cull, cull_min, cull_max; api_trace.hip: cull_box)
struct CullBox {
    int on = 0;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    bool operator==(const CullBox& o) const { return on == o.on && (on == 0 || (memcmp(lo, o.lo, sizeof lo) == 0 && memcmp(hi, o.hi, sizeof hi) == 0)); }
};
}  // namespace vxrt

using namespace vxrt;

struct vxrt_ctx {
    vxrt_config cfg{};
    BandMap band{};
    // Ownership: every member that is a DeviceBuf, PinnedBuf, Event or Stream (owned.h) is released by the context's destructor;
    // raw pointers and handles below are pieces or copies of an owned member and say so.  Members are destroyed in reverse order of
    // declaration, so the streams, declared here before everything else that owns, outlive every buffer and every event.
    Stream stream;
    std::vector<Stream> own_trace_streams;    // the trace streams of a context with inflight >= 2 (none with inflight == 1)
    std::vector<hipStream_t> trace_streams;   // handles, not owned: inflight entries; own_trace_streams, or `stream` when inflight == 1
    std::vector<Stream> aux_streams;          // one per trace stream, made on first use: the all-in-one grid of the longest tiles (VXRT_OPT_LONG_TILES)
    std::vector<Stream> low_streams;          // VXRT_OPT_TRACE_PRIORITY: one low-priority stream per trace stream
    Stream copy_stream;                       // vxrt_read_async

    // scene
    bool has_scene = false;
    DeviceBuf<SvoRecord> d_svo;               // with d_leaves and d_wide replaced only by replace_scene_arrays and commit_storage
    SvoRecord root_rec{0, 0};  // d_svo[0], passed to the kernels by value (every cast starts with it)
    DeviceBuf<WideRec> d_wide; // the same tree as wide records (kernels.h): two levels per 16-byte record
    WideRec wide_root{0, 0, 0, 0};
    size_t wide_count = 0;
    int scene_format = 0;      // VXRT_OPT_SCENE_FORMAT: 0 the 8-byte records (default), 1 also build and walk the wide records
    DeviceBuf<int32_t> d_leaves;
    size_t svo_count = 0, leaf_count = 0;
    float root_center[3] = {0, 0, 0};
    float root_size = 1.0f;
    // the sky cull's box (api_scene.hip: scene_box): every occupied cell of tree level min(depth, 7), world units, not yet grown
    bool box_valid = false;
    float box_min[3] = {0, 0, 0}, box_max[3] = {0, 0, 0};
    int sky_cull = 1;   // VXRT_OPT_SKY_CULL
    uint32_t depth = 0;
    DeviceBuf<float> d_noise;
    // in-place edits (api_edit.hip, vxrt_edit.h).  The first edit records how many records / leaf words the build produced: a block
    // below those counts is tight, one at or above them was allocated by an edit and holds 8 entries.  The storage grows only there.
    bool edited = false;
    size_t svo_built = 0, leaf_built = 0;
    size_t svo_cap = 0, leaf_cap = 0;   // entries allocated once an edit grew the storage (0: exactly svo_count / leaf_count)
    size_t live_nodes = 0;              // records in the tree (svo_count less the holes edits left: vxrt_stats.octree_nodes)
    // vxrt_get_voxels (api_extract.hip): the decode's scratch, grown on demand (never shrunk), released with the context
    struct GrowBuf { DeviceBuf<void> buf; size_t cap = 0; };   // cap: bytes
    struct ExtractScratch {
        GrowBuf front[2];   // frontier double buffer: uint4 {record, u.x, u.y, u.z} per node
        GrowBuf part;       // uint64 scan partials, one per block of the frontier, + the total
        GrowBuf pos, mrgb;  // output staging: int16[3] and 4 bytes per voxel
    };
    ExtractScratch extract;

    // Images (local rows x width, rgba32f).  The trace outputs live in a ring of frame slots so that the
    // trace stage of up to `inflight` consecutive frames can be on the GPU together (one stream each) while
    // the temporal/denoise stages run in frame order on `stream`.  A slot is not re-used while it still is
    // the temporal history or while a stage that reads it is in flight (slot.last_use).
    struct Slot {
        float4* sampled_color = nullptr;   // pieces of ring_arena, not owned
        float4* albedo = nullptr;
        float4* nd = nullptr;
        // Events.  A trace launch covers up to 32 slots and is ONE event (launch_events, per trace stream): recording two events
        // per slot cost ~8 us of host time per frame of a launch — more than a rank of 8 can afford (scripts/exp_host_submit.py).
        Event own;                        // recorded on the main stream by the stages that read the slot (temporal, denoise, halo pack, spp)
        hipEvent_t trace_done = nullptr;  // handle, not owned: the event of the launch that traced the slot
        hipEvent_t last_use = nullptr;    // handle: what must have finished before the slot is traced into again (`own` or a launch's event)
        bool last_use_recorded = false;
        // VXRT_OPT_SKY_ONCE: what the slot's all-sky tiles (first_hit_kernel: tile_sky) hold.  Set by a FULL trace launch that took its
        // first hits from the call's tagged records (finish_launch): those tiles then hold the sky of `cam` under this call's uniforms.
        // Whatever else writes one of the slot's three images inside a call clears it (vxrt_render_spp's average).  A tag of another
        // call is never honoured — the uniforms, the scene and the band cannot change inside one — so no setter has to know of it.
        struct SkyTag {
            uint64_t call = 0;    // call_id of the launch that stored the tiles (0: nothing known)
            Cam cam{};
            CullBox cull{};
            bool gbuf = false;    // normal/depth and albedo/node were stored with the colour
        };
        SkyTag sky;
    };
    std::vector<Slot> ring;
    int inflight = 1;
    DeviceBuf<char> ring_arena;               // the ring's images: one allocation (alloc_images)
    std::vector<Event> launch_events;    // two per trace stream, used alternately: "this launch has finished"
    std::vector<Event> head_events;      // one per trace stream: "this stream's last trace_kernel has finished" (VXRT_OPT_HEAD_STAGGER)
    std::vector<Event> aux_fork, aux_join;    // with aux_streams
    uint32_t long_tiles_permille = 0;         // 0: off
    int fused_tail = 0;                       // VXRT_OPT_FUSED_TAIL: head and compacted tail of a launch as one grid of persistent waves
    uint64_t fused_errors = 0;                // launches whose fused_kernel gave up a bounded wait (reported by vxrt_sync)
    int head_stagger = 0;                     // 1: a launch's head waits for the previous launch's head on another stream
    int last_head_lane = -1;
    std::vector<unsigned> launch_event_turn;
    int slot = 0;        // slot of the most recently traced frame
    int hist_slot = -1;  // slot whose normal/depth pairs with accum[hist] as the temporal history
    DeviceBuf<float4> accum[2];
    DeviceBuf<float4> denoised;
    DeviceBuf<float4> spp_sum;  // running sum of vxrt_render_spp (allocated on first use)
    // multi-rank halo (api_halo.hip): the rows of the neighbouring ranks just outside this rank's bands, as last unpacked
    DeviceBuf<float4> halo;            // store: two messages (kernels.h: HaloView)
    size_t halo_store_f4 = 0;          // its size in float4
    HaloView halo_view{nullptr, 0, 0, 0, 0};   // what the store holds right now (rows = 0: nothing)
    uint32_t halo_min_rows = 1;        // VXRT_OPT_HALO_ROWS: rows that travel even without a denoise window (temporal's reprojection)
    bool halo_valid = false;           // the store holds the current frame's rows (cleared by the next trace)
    Event halo_event;                  // vxrt_stream_wait_context / vxrt_context_wait_stream
    DeviceBuf<uint16_t> d_tile_rows;   // denoise tile rows: [interior..., edge...] (those that need no halo, those that do)
    uint32_t tile_rows_interior = 0, tile_rows_edge = 0;
    uint64_t temporal_count = 0;       // temporal stages run so far ...
    uint64_t halo_epoch = ~0ull;       // ... and its value when the halo was last imported: equal -> the halo holds the
                                       // neighbours' rows of the current temporal history
    int cur = 0;             // accum[cur] is written by the next temporal stage, accum[cur^1] is the history
    bool has_history = false;
    bool accum_is_sampled = true;  // the latest "accumulated" image is sampled_color (temporal never ran)
    int last = 0;                   // index of the most recently written accum image
    uint64_t traced = 0;            // frames traced so far
    uint64_t trace_launches = 0;    // trace launches so far (selects the trace stream)
    uint64_t timed_launches = 0;
    int batch = 1;                  // vxrt_config.frames_per_launch

    // parameters
    vxrt_uniforms uniforms{};
    vxrt_temporal temporal{};
    vxrt_denoise denoise{};
    float cam_pos[3] = {0, 0, -2}, cam_dir[3] = {0, 0, 1}, cam_fov = 1.2217305f;  // src/context.rs:618-622
    Cam cam{}, old_cam{};
    bool old_cam_valid = false;

    // stats
    DeviceBuf<unsigned long long> d_rays;
    // wavefront tracer: two path queues (ping-pong) and three rotating sets of 64 shard counters
    struct StreamQueues {  // per trace stream; allocated only for the queue-based variants
        DeviceBuf<float4> hitq[2];              // sharded PathRec queues (variant 2: ping-pong; variant 3: [0] = primary hits)
        DeviceBuf<unsigned> counts3;            // three rotating sets of 64 shard counters
        unsigned launches = 0;
        RayQueue rq{};                          // variant 3: pointers into rq_block, not owned
        DeviceBuf<char> rq_block;
        // tail queue sized by need (variants 4 / 5): the counters trace_kernel wrote, copied back after every launch
        PinnedBuf<unsigned> host_counts;        // pinned, one set: 64 counters, 16 uints apart
        Event counts_ready;
        bool counts_pending = false;
        unsigned counts_capacity = 0;           // the shard capacity of the launch whose counters host_counts holds
        // fused head + tail (VXRT_OPT_FUSED_TAIL; trace.hip: fused_kernel)
        DeviceBuf<char> fused_ctl;              // the launch's cursors, zeroed on the stream before every launch
        PinnedBuf<unsigned> host_ctl;           // pinned: the first 16 bytes of fused_ctl after a launch (word 2: a bounded wait ran out)
        bool stamps_clean = false;              // every record slot of hitq[0] carries stamp 0 (set when the queue is cleared, lost when it is re-allocated)
        unsigned fused_launches = 0;            // -> the launch's stamp, 1 .. 65535
    };
    std::vector<StreamQueues> queues;
    unsigned shard_capacity = 0;        // records per shard of the path queues
    unsigned shard_capacity_max = 0;    // ... in the worst case: every pixel of every frame of a launch hands its path over
    int tail_capacity_override = 0;     // test hook (VXRT_TAIL_CAPACITY / vxrt_set_option): > 0 pins the capacity
    uint64_t queue_overflow_paths = 0;  // paths that found their shard full and stayed in the head kernel
    uint64_t queue_bytes = 0;
    int denoise_mode = 0;               // VXRT_OPT_DENOISE_MODE: 0 exact (bit-identical to the oracle), 1 tolerant (post.hip)
    // 0 = monolithic trace_kernel (all bounces in one launch; default), 2 = wavefront launches per path segment,
    // 3 = ray queues: shade / trace launches with per-lane ray refill
    int trace_variant = 0;
    // tracer 0 (auto): scenes that do not fit the 256 MB Infinity Cache use the all-in-one kernel — compacting paths trades
    // the locality of a tile's rays for lane utilisation, which loses once SVO gathers go to HBM (config 5, 5.6 GiB:
    // 2.29 vs 3.30 ms per 4K frame)
    bool auto_tracer = false;
    int shade_blocks = 1024;
    unsigned rays_per_wave = 256;  // ray-queue tracer: fewest rays a trace wave takes (more = better lane refill, fewer waves)
    // longest-tile-first scheduling of the monolithic kernel: cost of every 16x16 tile in the last frame -> order
    struct TileSchedule {  // one per trace stream: costs of the frame it traced last, and the order made from them
        DeviceBuf<uint32_t> cost;
        DeviceBuf<uint32_t> order;
        DeviceBuf<uint32_t> last_cost;  // copy for diagnostics (vxrt_debug_tile_costs)
        DeviceBuf<uint32_t> scratch;    // per-block histograms of the sort (256 x 128)
        bool valid = false;
        int age = 0;  // frames traced since the last sort
        // VXRT_OPT_TRACE_PRIORITY: how many tiles of `order` walk (they come first: the order is plain longest-first then), read back
        // after every sort; 0 = not known (yet): the launch goes out as one grid
        PinnedBuf<unsigned> host_heavy;     // pinned
        Event heavy_ready;
        bool heavy_pending = false;
        unsigned heavy = 0;
    };
    std::vector<TileSchedule> schedules;
    int last_schedule = 0;
    int use_tile_order = 1;
    int trace_blocks = 2048;
    int spread_override = -1;     // VXRT_OPT_TILE_SPREAD (tests, experiments): see launch_tile_order
    int node_order = 0;           // VXRT_OPT_NODE_ORDER: 2 / 3 = depth-first treelets of the last 2 / 3 node levels (scene_device.hip)
    int node_order_applied = 0;   // ... and whether the scene in place was reordered (vxrt_stats.node_order)
    int host_scene_build = 0;     // VXRT_OPT_HOST_SCENE_BUILD: vxrt_set_menger builds on the host even where the device builder could
    unsigned wave_slots = 5120;   // waves of trace_kernel the device holds at once: CUs x 4 SIMDs x 5 (vxrt_create)
    int frame_lanes = 1;   // trace_kernel may put 8 frames of a pixel row into a wave (TraceArgs::frame_lanes; VXRT_OPT_FRAME_LANES)
    uint32_t frame_lane_launches = 0;
    // VXRT_OPT_SHARED_PRIMARY: a launch of >= 2 frames of ONE camera takes each pixel's first hit from a record (trace.hip:
    // first_hit_kernel).  1: every such launch walks the primary rays itself; 2: one walk per API call serves all its launches that
    // have the walk's camera and cull state (first_hit_tag)
    int shared_primary = 2;
    uint64_t shared_primary_launches = 0;   // vxrt_debug_shared_primary_launches: launches that took their first hits from records
    uint64_t first_hit_walks = 0;           // vxrt_debug_first_hit_walks: launches of first_hit_kernel
    std::vector<DeviceBuf<uint4>> first_hits;         // per trace stream: one 16-byte record per pixel of the band (contexts with frames_per_launch >= 2)
    std::vector<Event> first_hit_walked;              // per buffer of first_hits: recorded behind the walk that filled it (option 2)
    // [buffer * inflight + stream]: the event (a handle to one of launch_events, or null) of the last launch on `stream` that read
    // `buffer` and that no later walk into the buffer has waited for yet
    std::vector<hipEvent_t> first_hit_readers;
    // The API call in progress: bumped on entry by vxrt_render, vxrt_render_frames, vxrt_render_path and vxrt_render_spp.  Neither the
    // scene nor the band nor an option can change inside one, so what a launch of the call computed from them holds for the call's rest.
    uint64_t call_id = 0;
    // What the records of the last walk under option 2 were made from.  They are valid for the call that made them only: no mutator
    // of the scene, the camera or an option has to know of them.
    struct FirstHitTag {
        uint64_t call = 0;      // call_id of the walk (0: no records)
        size_t buffer = 0;      // index into first_hits = the trace stream that walked
        Cam cam{};              // the camera the rays were made from
        CullBox cull{};         // the sky cull the walk used: a culled lane wrote no record
        uint64_t walk = 0;      // which walk of the context it was (walk_serial): a WalkList made from an earlier one is stale
        bool sky = false;       // the walk noted the all-sky tiles (tile_sky[buffer]) and sent their numbers off (sky_count): VXRT_OPT_SKY_ONCE
    };
    FirstHitTag first_hit_tag;
    uint64_t walk_serial = 0;   // walks of the primary rays issued so far (never reset)
    // VXRT_OPT_SKY_ONCE (default 1): inside one API call, a launch whose slots all hold this call's sky already (Slot::sky) goes out
    // over the tiles that walk alone — same kernel, same blocks for those tiles — and the rays of the pixels left out are counted on
    // the host (sky_rays).  0: every launch covers every tile, as before the option existed.
    int sky_once = 1;
    bool sky_tiles = false;             // trace_kernel's tiles are first_hit_kernel's 8 x 8 pixels (alloc_images)
    uint64_t call_frames = 0;           // frames the API call in progress traces: one that goes less than twice round the ring asks for no flags and no list
    std::vector<DeviceBuf<uint32_t>> tile_sky;        // per buffer of first_hits, written by the same walk and valid under the same tag
    struct WalkList {   // per trace stream: the stream's launch order without the all-sky tiles (trace.hip: walk_list_kernel)
        DeviceBuf<uint32_t> order;      // the first SkyCount::n_walk entries
        DeviceBuf<uint32_t> partial;    // the kernels' scratch; its last two words are the list's numbers
        uint64_t order_walk = 0;        // FirstHitTag::walk the list in `order` was made from (0: none, or the stream's order has changed since)
    };
    std::vector<WalkList> walk_lists;
    // How many tiles walk, and how many pixels the others have: numbers of the WALK, the same on every stream.  They leave with the
    // walking launch's own list, right behind first_hit_kernel, and are on the host long before the call comes back to a ring slot.
    struct SkyCount {
        PinnedBuf<unsigned> host;       // pinned: {tiles that walk, pixels of the tiles that do not}
        Event ready;                    // behind the copy into host
        bool pending = false;
        uint64_t pending_walk = 0;      // FirstHitTag::walk the numbers under way belong to
        uint64_t walk = 0;              // ... n_walk and skipped_pixels belong to (0: none)
        unsigned n_walk = 0, skipped_pixels = 0;
    };
    SkyCount sky_count;
    uint64_t sky_rays = 0;              // primary rays of pixels that thin launches left out (vxrt_stats.rays adds them to the device's count)
    uint64_t thin_launches = 0;         // vxrt_debug_thin_launches
    uint64_t trace_kernel_blocks = 0;   // vxrt_debug_trace_blocks: blocks of trace_kernel issued, summed over the launches
    int path_blocks = 512;  // tracer 5: blocks of path_kernel (each wave takes an equal range of the queue, >= 512 paths)
    int tail_from = 1;  // tracer 4: the hit number at which live paths move to the compacted launches
    unsigned tail_split = 0;  // ... bit k: the tail compacts again and starts a new launch at path segment k
    unsigned trace_split = 0x1;  // bit k: compact live paths and start a new launch at path segment k
    uint64_t frames = 0, pixels = 0, timed_frames = 0;
    double ms[5] = {0, 0, 0, 0, 0};   // trace, temporal, denoise, halo pack, halo unpack
    uint64_t halo_exchanges = 0;
    std::vector<EventPair> pending, free_pairs;
    std::vector<Event> pair_events;   // every event take_pair made: the pairs above are handles to them

    // vxrt_read_async (api_context.hip): a copy stream of the context's own, two slots; a slot = a device-side snapshot of the image
    // (so that later frames may overwrite the image while the snapshot travels) + "snapshot taken" / "transfer arrived" events
    struct ReadSlot {
        DeviceBuf<char> stage;
        size_t stage_bytes = 0;
        Event snap, arrived;
        bool in_flight = false;
    };
    ReadSlot read_slots[2];
    // the displayed frame (vxrt_device_image / vxrt_read of VXRT_DISPLAY_*): 4 bytes per pixel, allocated on first use, freed with the images
    DeviceBuf<uint32_t> display;

    // VXRT_OPT_TRACE_PRIORITY (round 6's experiment): the trace streams at the device's highest priority, the tiles that only store
    // sky as a grid of their own on a low-priority stream per trace stream
    int trace_priority = 0;
    int xcd_affinity = 0;               // VXRT_OPT_XCD_AFFINITY: 0 off, S = side of a super-tile in tiles (api_trace.hip: xcd_affine_order)
    unsigned xcd_balance_permille = 0;  // (max - min) / max of the 8 lists' summed costs at the last such sort
    uint64_t split_launches = 0;        // trace launches that went out as two grids
    std::vector<Event> low_fork, low_join;   // with low_streams

    int morph_tile_lookup = 0;    // vxrt_debug_morph_tile_lookup: vxrt_morph_voxels_device asks the block's LDS tile before the whole array

    // touch map (vxrt_debug_touch_map; -DVXRT_VARIANTS=1 builds): one bit per 64-byte line of the node records / the leaf words
    DeviceBuf<uint32_t> d_touch_nodes;
    DeviceBuf<uint32_t> d_touch_leaves;
    size_t touch_node_lines = 0, touch_leaf_lines = 0;
    // the DDA prototype's grid of the scene in place (vxrt_debug_dda_rays; -DVXRT_VARIANTS=1 builds): bricks, brick bits, super-brick bits, first leaf per brick
    DeviceBuf<void> dda_grid[4];
    int dda_levels = 0;
};

namespace vxrt {
// ---- the plan of one trace launch: every decision about it, made once by plan_trace and carried out by trace_frames (api_trace.hip)
constexpr size_t kInfinityCacheBytes = size_t(256) << 20;   // a scene larger than this waits for HBM: compared in ONE place, TracePlan::hbm
// tracers (internal numbers) that take several frames per launch: the all-in-one kernel (0) and the head + tail pairs (4, 5)
inline bool batches_frames(int tracer) { return tracer == 0 || tracer >= 4; }
enum class TracePath { all_in_one, head_bounces, head_paths, fused, wavefront, ray_queue };   // trace_kernel | + bounce_kernel | + path_kernel | fused_kernel | tracers 2, 3
enum class TileSort { none, longest_first, xcd_affine };
struct TracePlan {
    bool hbm;                  // the scene is beyond the Infinity Cache: trace_kernel's instantiation for it, the all-in-one schedule under tracer auto
    bool wide_head, wide_tail; // the head / the tail walks the wide records
    int tracer;                // the tracer that really runs: 0 where auto falls back to the all-in-one kernel, else vxrt_ctx::trace_variant
    TracePath path;
    int frame_lanes;           // frames a wave of the head holds, as the kernel really uses it (TraceArgs::frame_lanes): 8, 4 or 0
    bool share;                // the frames take their first hits from records (vxrt_ctx::first_hits[hits]) ...
    bool walk;                 // ... which this launch's own first_hit_kernel writes; false: an earlier launch of the call has
    size_t hits;               // the buffer of the records: this launch's stream when it walks, else the stream that did
    unsigned long_blocks;      // blocks of the longest tiles that go out as a grid of their own (0: none); the head starts behind them
    bool single_tail_launch;   // the tail is exactly one launch: the counter copy-back goes behind it
    unsigned split_heavy;      // priority split: the first split_heavy tiles of the order on the trace stream, the rest on the low-priority one (0: one grid)
    bool thin;                 // sky once: trace_kernel goes out over the stream's WalkList alone, n_walk tiles (every slot holds its sky already)
    unsigned n_walk;           // ... their number, and the pixels per frame that are left out and counted on the host
    unsigned skipped_pixels;
    bool stamps_sky;           // a full launch that leaves this call's sky in its slots' all-sky tiles: finish_launch tags the slots
    TileSort sort;             // how this launch re-sorts the stream's tiles when it is over
};

// the DDA prototype's grid was built from records that are about to change, or have (vxrt_debug_dda_rays builds it again)
inline void drop_dda_grid(vxrt_ctx* c) {
    for (DeviceBuf<void>& g : c->dda_grid) g.reset();
    c->dda_levels = 0;
}
// a new scene: the touch maps were sized for the old one (vxrt_debug_touch_map), and so was the DDA prototype's grid
inline void drop_touch_maps(vxrt_ctx* c) {
    c->d_touch_nodes.reset();
    c->d_touch_leaves.reset();
    c->touch_node_lines = c->touch_leaf_lines = 0;
    drop_dda_grid(c);
}
// a scene was just set (api_scene.hip): none of it comes from an edit
inline void scene_replaced(vxrt_ctx* c) {
    c->edited = false;
    c->svo_built = c->leaf_built = c->svo_cap = c->leaf_cap = 0;
    c->live_nodes = c->svo_count;
}
// ---- api_context.hip
size_t image_bytes(const vxrt_ctx* c);
int count_local_rows(const BandMap& b);
int local_band_count(const BandMap& b);
void free_images(vxrt_ctx* c);
int alloc_images(vxrt_ctx* c);
int sync_all(vxrt_ctx* c);
int set_band(vxrt_ctx* c, uint32_t width, uint32_t height);
EventPair take_pair(vxrt_ctx* c, int stage);
int resolve_events(vxrt_ctx* c);
bool valid_ctx(const vxrt_ctx* c);
float4* image_ptr(vxrt_ctx* c, vxrt_image which);
bool is_display(vxrt_image which);                    // VXRT_DISPLAY_BGRA8_SRGB / VXRT_DISPLAY_RGBA8_SRGB
size_t display_bytes(const vxrt_ctx* c);              // local_rows * width * 4
// ---- api_scene.hip
bool use_wide(const vxrt_ctx* c);
// the smallest box of cells of tree level min(depth, 7) that holds every voxel; recs: the first records of the tree, breadth first,
// at least those of levels 0 .. min(depth, 7) - 1.  false: no voxel at all
bool scene_box(const SvoRecord* recs, size_t count, uint32_t depth, const float root_center[3], float root_size, float box_min[3], float box_max[3]);
// the same box for breadth-first records in device memory (root = svo[0]): reads the prefix back.  *valid as scene_box's result
int device_scene_box(const SvoRecord* svo, size_t nsvo, uint32_t depth, SvoRecord root, const float root_center[3], float root_size, bool* valid,
                     float box_min[3], float box_max[3]);
// The one way the scene's arrays are replaced: takes ownership of the new ones (any may be empty), releases the old, sets the counts,
// and drops what was sized for or built from the old records (the touch maps, the DDA grid).  The root, the box, the capacities and
// scene_replaced stay with the caller.
void replace_scene_arrays(vxrt_ctx* c, DeviceBuf<SvoRecord>&& svo, size_t nsvo, DeviceBuf<int32_t>&& leaves, size_t nleaves, DeviceBuf<WideRec>&& wide,
                          size_t nwide);
// device arrays built for the context become its scene (sets the counts, the sky cull's box, the node order)
int install_scene(vxrt_ctx* c, DeviceBuf<SvoRecord>&& svo, size_t nsvo, DeviceBuf<int32_t>&& lw, size_t nlw, uint32_t depth, SvoRecord root,
                  DeviceBuf<WideRec>&& wide, size_t nwide, WideRec wide_root);
int widen_svo(const std::vector<SvoRecord>& recs, uint32_t depth, std::vector<WideRec>* out);
// ---- api_trace.hip
int resize_tail_queues(vxrt_ctx* c, unsigned want);
int apply_option(vxrt_ctx* c, uint32_t option, uint32_t value, bool at_create);   // api_context.hip
CullBox cull_box(const vxrt_ctx* c, const Cam* cams, uint32_t g);                  // api_trace.hip
void set_cull(TraceArgs& a, const CullBox& b);
int grow_tail_queues(vxrt_ctx* c, size_t lane);
void update_bindings(vxrt_ctx* c);
void frame_constants(const vxrt_ctx* c, TraceArgs& a);
int trace_frames(vxrt_ctx* c, uint32_t g, bool timed, int* slots, Cam* cams, Cam* olds, const float (*path_pos)[3] = nullptr,
                 const float (*path_dir)[3] = nullptr, uint32_t gbuf_frames = 0xffffffffu);
// ---- api_frame.hip
int check_render(vxrt_ctx* c, uint32_t flags);
int post_stages(vxrt_ctx* c, uint32_t flags, bool timed);
// ---- api_halo.hip
void free_halo(vxrt_ctx* c);            // the halo store and the tile rows, with their bookkeeping
int build_tile_rows(vxrt_ctx* c);       // after the band map changed
uint32_t halo_rows_wanted(const vxrt_ctx* c);   // rows per band edge the next exchange carries
}  // namespace vxrt
