// api_trace.hip — scheduling of the trace stage of libvxrt: which ring slots, stream, tile order and tail queue a launch of
// trace_kernel (+ bounce_kernel) gets, for 1..32 consecutive frames per launch and several launches in flight.
#include <algorithm>
#include <cmath>

#include "ctx.h"
#include "vx_vec.h"

namespace vxrt {

// new capacity (records per shard) for the path queues of every stream; waits for the GPU first.  All new buffers are allocated before
// any old one is released: if an allocation fails the context keeps its queues, its capacity and its accounting as they were.
int resize_tail_queues(vxrt_ctx* c, unsigned want) {
    want = want > c->shard_capacity_max ? c->shard_capacity_max : (want + 63u) / 64u * 64u;
    if (want == c->shard_capacity) return VXRT_OK;
    if (int rc = sync_all(c)) return rc;
    const size_t new_bytes = (size_t(want) * 64 + 1) * 64, old_bytes = (size_t(c->shard_capacity) * 64 + 1) * 64;
    std::vector<DeviceBuf<float4>> fresh;
    for (vxrt_ctx::StreamQueues& q : c->queues)
        for (DeviceBuf<float4>& p : q.hitq)
            if (p) {
                fresh.emplace_back();
                if (hipError_t e = fresh.back().alloc(new_bytes / sizeof(float4)); e != hipSuccess) return hip_fail(e, "hipMalloc (tail queues)");
            }
    size_t k = 0;
    for (vxrt_ctx::StreamQueues& q : c->queues)
        for (DeviceBuf<float4>& p : q.hitq)
            if (p) {
                p.swap(fresh[k++]);   // the old queue goes with `fresh`
                c->queue_bytes += new_bytes - old_bytes;
            }
    c->shard_capacity = want;
    for (vxrt_ctx::StreamQueues& q : c->queues) q.stamps_clean = false;   // fresh memory: fused_kernel's stamps must be cleared before its next launch
    return VXRT_OK;
}

// Tail queues sized by need: look at what the stream's last launch wanted (its shard counters, copied back after the launch, with the
// capacity that launch ran with) and, if that did not fit, make the queues larger before the stream's next launch.  Paths that did not
// fit were followed by the head kernel itself, so no frame was wrong — only slower.
int grow_tail_queues(vxrt_ctx* c, size_t lane) {
    vxrt_ctx::StreamQueues& sq = c->queues[lane];
    if (!sq.counts_pending || hipEventQuery(sq.counts_ready) != hipSuccess) return VXRT_OK;
    sq.counts_pending = false;
    if (sq.host_ctl != nullptr && sq.host_ctl[2] != 0u) { c->fused_errors++; sq.host_ctl[2] = 0u; }
    unsigned peak = 0;
    for (unsigned s = 0; s < 64; s++) {
        const unsigned n = sq.host_counts[s * 16];
        peak = n > peak ? n : peak;
        if (n > sq.counts_capacity) c->queue_overflow_paths += n - sq.counts_capacity;   // against the capacity THAT launch had
    }
    if (peak <= c->shard_capacity || c->tail_capacity_override > 0 || c->shard_capacity >= c->shard_capacity_max) return VXRT_OK;
    // every stream's queues share one capacity (PathQueue::shard_capacity travels with the launch): grow them all, at rest
    unsigned want = peak + peak / 4u;
    want = want < 2u * c->shard_capacity ? 2u * c->shard_capacity : want;
    return resize_tail_queues(c, want);
}

Cam make_cam(const float pos[3], const CameraBasis& b) {
    Cam c;
    for (int i = 0; i < 3; i++) { c.o[i] = pos[i]; c.r[i] = b.right[i]; c.u[i] = b.up[i]; c.f[i] = b.forward_ray[i]; }
    return c;
}


// Context::update_bindings for one frame (src/context.rs:2136-2162): old <- current, current <- camera, frame_number + 1
void update_bindings(vxrt_ctx* c) {
    c->old_cam = c->cam;
    CameraBasis basis = camera_axis_scaled(c->cam_dir, c->cam_fov, c->cfg.width, c->cfg.height);
    c->cam = make_cam(c->cam_pos, basis);
    for (int i = 0; i < 3; i++) {
        c->uniforms.camera_origin[i] = c->cam.o[i]; c->uniforms.camera_right[i] = c->cam.r[i];
        c->uniforms.camera_up[i] = c->cam.u[i]; c->uniforms.camera_forward[i] = c->cam.f[i];
    }
    c->uniforms.still_sample += 1;
    c->uniforms.frame_number += 1;  // wrapping
}

// The fields of TraceArgs that depend on the scene and the uniforms only (not on the frame slots or the launch).
void frame_constants(const vxrt_ctx* c, TraceArgs& a) {
    const vxrt_uniforms& u = c->uniforms;
    a.svo = c->d_svo; a.leaves = c->d_leaves; a.noise = c->d_noise;
    a.root_rec = c->root_rec;
    a.wide = c->d_wide;
    a.wide_root = c->wide_root;
    a.node_levels = int(c->depth) + 1;
    memcpy(a.root_center, c->root_center, sizeof a.root_center);
    a.root_size = c->root_size;
    a.band = c->band;
    a.max_bounces = int(c->cfg.max_bounces);
    a.launch_index = 0;
    a.block_first = 0;
    a.cull = 0;
    a.first_hit = nullptr;
    a.tile_sky = nullptr;
    a.stack_levels = c->depth < 1 ? 1 : int(c->depth);
#if VXRT_VARIANTS
    a.touch_nodes = c->d_touch_nodes;
    a.touch_leaves = c->d_touch_leaves;
#endif
    // voxels.comp:296 and the other per-frame constants, evaluated once with the same operations
    f3 sun_dir = mk3(vx_cos(u.sun_yaw) * vx_cos(u.sun_pitch), -vx_sin(u.sun_pitch), vx_sin(u.sun_yaw) * vx_cos(u.sun_pitch));
    f3 sun_n = norm3(sun_dir), neg_sun_n = norm3(-sun_dir);
    f3 sun_color = u.sun_strength * mk3(u.sun_color[0], u.sun_color[1], u.sun_color[2]);
    a.sun_dir[0] = sun_dir.x; a.sun_dir[1] = sun_dir.y; a.sun_dir[2] = sun_dir.z;
    a.sun_dir_n[0] = sun_n.x; a.sun_dir_n[1] = sun_n.y; a.sun_dir_n[2] = sun_n.z;
    a.neg_sun_dir_n[0] = neg_sun_n.x; a.neg_sun_dir_n[1] = neg_sun_n.y; a.neg_sun_dir_n[2] = neg_sun_n.z;
    a.sun_color[0] = sun_color.x; a.sun_color[1] = sun_color.y; a.sun_color[2] = sun_color.z;
    a.sky_color[0] = u.sky_color[0]; a.sky_color[1] = u.sky_color[1]; a.sky_color[2] = u.sky_color[2];
    a.sun_exponent = 1.0f / (u.sun_size * u.sun_size);
    // vx_pow(x, y) = vx_exp(y * vx_log(x)) is +0 once y * log(x) < -87.3: certain for x < exp(-88 / y) * (1 - 1e-4), which leaves
    // 0.7 + 1e-4 y of margin in the exponent against vx_log's error of ~1e-6 |log x| and the product's rounding.
    a.sun_zero_below = 0.0f;
    if (a.sun_exponent > 1.0f && a.sun_exponent < 1e6f) a.sun_zero_below = float(exp(-88.0 / double(a.sun_exponent)) * (1.0 - 1e-4));
    a.sun_size = u.sun_size; a.sun_strength = u.sun_strength; a.emit_strength = u.emit_strength; a.specularity = u.specularity;
}

// Sky cull: the scene's box grown by a margin m that dwarfs every rounding error of the walk and of the test itself.  The walk
// visits a cell only if the ray passes within ~2^-21 (|origin| + root_size) of it (its plane times are fl(fl(p - o) * inv): two
// roundings of quantities no larger than that); m = 0.01 + 2^-16 (max |origin| + 2 root_size) is at least 32 times as much.
CullBox cull_box(const vxrt_ctx* c, const Cam* cams, uint32_t g) {
    CullBox b;
    if (c->sky_cull && c->box_valid) {
        float far = 0.0f;
        bool sane = true;
        for (uint32_t k = 0; k < g; k++)
            for (int i = 0; i < 3; i++) {
                const float v = fabsf(cams[k].o[i]);
                sane = sane && v < 1e6f && std::isfinite(cams[k].r[i]) && std::isfinite(cams[k].u[i]) && std::isfinite(cams[k].f[i]);   // NaN fails v < 1e6
                far = v > far ? v : far;
            }
        if (sane) {
            const float m = 0.01f + ldexpf(far + 2.0f * c->root_size, -16);
            for (int i = 0; i < 3; i++) { b.lo[i] = c->box_min[i] - m; b.hi[i] = c->box_max[i] + m; }
            b.on = 1;
        }
    }
    return b;
}

void set_cull(TraceArgs& a, const CullBox& b) {
    a.cull = b.on;
    for (int i = 0; i < 3; i++) { a.cull_min[i] = b.lo[i]; a.cull_max[i] = b.hi[i]; }
}

// VXRT_OPT_XCD_AFFINITY (round 6's experiment for scenes that live in HBM, BASELINE config 5): a launch order in which the tiles that
// walk reach the XCDs by SCREEN REGION instead of round robin.  Blocks are dealt to the 8 XCDs in turn (block b and b + 8 share one:
// observed, not promised — a wrong guess costs speed only), every XCD has an L2 of its own, and neighbouring tiles read neighbouring
// parts of the tree: dealt round robin, each XCD fetches its own copy of every line (config 5 from outside: 9.8 x the unique bytes
// of a frame come in from beyond the L2s, 31 x inside a tunnel — bench.py: extra.config5_*.roofline.refetch).  So: the screen in
// super-tiles of S x S tiles; each super-tile's walking tiles belong to ONE of 8 lists, the super-tiles dealt longest first to the list
// with the least summed cost so far (the measured tile costs: the lists end up within a few per cent of each other, which matters
// because the dispatcher's round robin waits for the slowest XCD); every list longest first; order[8 i + x] = list x's i-th tile, a
// list that has run out filled up with tiles of sky (no scene traffic: any XCD may have them), or with the shortest chains of the
// longest list when there is no sky left; what remains of the sky comes last.  Made on the HOST from the costs copied back (a stall
// of its own every 8th launch: an experiment's price), one frame per launch only.
static int xcd_affine_order(vxrt_ctx* c, vxrt_ctx::TileSchedule& sched, hipStream_t ts) {
    const unsigned tiles = trace_tile_count(c->band.width, c->band.local_rows);
    int tw = 8, th = 8;
    trace_tile_dims(&tw, &th);
    const unsigned tx = unsigned(c->band.width + tw - 1) / unsigned(tw), ty = tiles / (tx ? tx : 1u);
    const unsigned S = unsigned(c->xcd_affinity);
    std::vector<uint32_t> cost(tiles), order;
    order.reserve(tiles);
    HIP_TRY(hipStreamSynchronize(ts));
    HIP_TRY(hipMemcpy(cost.data(), sched.cost, size_t(tiles) * 4, hipMemcpyDeviceToHost));
    const unsigned sx = (tx + S - 1) / S, sy = (ty + S - 1) / S;
    std::vector<unsigned long long> scost(size_t(sx) * sy, 0ull);
    for (unsigned t = 0; t < tiles; t++)
        if (cost[t] >= 4u) scost[size_t(t / tx / S) * sx + (t % tx) / S] += cost[t];
    std::vector<unsigned> supers(scost.size());
    for (unsigned i = 0; i < supers.size(); i++) supers[i] = i;
    std::stable_sort(supers.begin(), supers.end(), [&](unsigned a, unsigned b) { return scost[a] > scost[b]; });
    std::vector<int> owner(scost.size(), 0);
    unsigned long long load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (unsigned s : supers) {
        int best = 0;
        for (int x = 1; x < 8; x++) if (load[x] < load[best]) best = x;
        owner[s] = best;
        load[best] += scost[s];
    }
    std::vector<uint32_t> lists[8], sky;
    for (unsigned t = 0; t < tiles; t++) {
        if (cost[t] >= 4u) lists[owner[size_t(t / tx / S) * sx + (t % tx) / S]].push_back(t);
        else sky.push_back(t);
    }
    for (auto& l : lists) std::stable_sort(l.begin(), l.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    size_t head[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tail[8], sky_next = 0;
    for (int x = 0; x < 8; x++) tail[x] = lists[x].size();
    auto left = [&](int x) { return tail[x] - head[x]; };
    for (;;) {
        bool any = false;
        for (int x = 0; x < 8; x++) any = any || left(x) != 0;
        if (!any) break;
        for (int x = 0; x < 8; x++) {
            if (left(x) != 0) { order.push_back(lists[x][head[x]++]); continue; }
            if (sky_next < sky.size()) { order.push_back(sky[sky_next++]); continue; }
            int longest = -1;                               // no sky left: the cheapest tile of the list with the most left
            for (int y = 0; y < 8; y++) if (left(y) > 1 && (longest < 0 || left(y) > left(longest))) longest = y;
            if (longest >= 0) order.push_back(lists[longest][--tail[longest]]);
            // else: nothing to pad with — this slot is skipped (the launch's last blocks; the lists that still hold a tile follow in this round)
        }
    }
    while (sky_next < sky.size()) order.push_back(sky[sky_next++]);
    if (order.size() != tiles) { set_error("xcd_affine_order: internal error (order incomplete)"); return VXRT_E_INVALID; }
    HIP_TRY(hipMemcpy(sched.order, order.data(), size_t(tiles) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(sched.last_cost, cost.data(), size_t(tiles) * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemsetAsync(sched.cost, 0, size_t(tiles) * 4, ts));
    unsigned long long lo = load[0], hi = load[0];
    for (int x = 1; x < 8; x++) { lo = load[x] < lo ? load[x] : lo; hi = load[x] > hi ? load[x] : hi; }
    c->xcd_balance_permille = hi ? unsigned((hi - lo) * 1000ull / hi) : 0u;
    return VXRT_OK;
}

// ---- the trace launch: what plan_trace decided (ctx.h: TracePlan), issued by one function per path -------------------------------

// The three counter sets of a stream rotate as in launch_trace_wavefront: launch J reads set J % 3, writes (J + 1) % 3, clears (J + 2) % 3.
struct CountSets {
    unsigned* sets[3] = {nullptr, nullptr, nullptr};
    unsigned J = 0;
    CountSets() = default;
    explicit CountSets(const vxrt_ctx::StreamQueues& sq) : sets{sq.counts3, sq.counts3 + 64 * 16, sq.counts3 + 2 * 64 * 16}, J(sq.launches) {}
    unsigned* read() const { return sets[J % 3]; }
    unsigned* written() const { return sets[(J + 1) % 3]; }
    unsigned* cleared() const { return sets[(J + 2) % 3]; }
};

// one launch: what its steps share.  cull, plan, a and counts are filled by the steps named after them, in that order
struct TraceLaunch {
    vxrt_ctx* c; hipStream_t ts; size_t lane; uint32_t g; const int* slots;
    CullBox cull{};     // the launch's sky cull (cull_box), as the plan compared it and the kernels get it
    TracePlan plan{};
    TraceArgs a;
    CountSets counts;   // the stream's counter sets as this launch finds them (tracers with queues)
    TraceLaunch(vxrt_ctx* c_, hipStream_t ts_, size_t lane_, uint32_t g_, const int* slots_) : c(c_), ts(ts_), lane(lane_), g(g_), slots(slots_) {}
};

// A camera path: the frames of a wave have cameras of their own, and what they share shrinks with the image motion across a group of
// F frames — estimated in pixels from the poses (rotation, and translation seen from the scene's centre), the worst group's.  NaN poses
// give NaN.  Measured on an orbit of the bench scene: + 4 % at 0.16-0.4 degrees (2-5 pixels) per 8 frames, + 2 % at 0.8 (11 pixels),
// - 1 % at 1.6 (21), - 3 % at 4 degrees (55)
static float path_motion_px(const vxrt_ctx* c, uint32_t g, uint32_t F, const float (*path_pos)[3], const float (*path_dir)[3]) {
    const float f_px = 0.5f * float(c->cfg.height) / tanf(0.5f * c->cam_fov);
    float worst = 0.0f;
    for (uint32_t k = 0; k + F <= g; k += F) {
        const float* p0 = path_pos[k]; const float* p1 = path_pos[k + F - 1];
        const float* d0 = path_dir[k]; const float* d1 = path_dir[k + F - 1];
        const float n0 = sqrtf(d0[0] * d0[0] + d0[1] * d0[1] + d0[2] * d0[2]), n1 = sqrtf(d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2]);
        float cosang = (d0[0] * d1[0] + d0[1] * d1[1] + d0[2] * d1[2]) / (n0 * n1);
        cosang = cosang > 1.0f ? 1.0f : (cosang < -1.0f ? -1.0f : cosang);
        const float ang = acosf(cosang);
        const float dp = sqrtf((p1[0] - p0[0]) * (p1[0] - p0[0]) + (p1[1] - p0[1]) * (p1[1] - p0[1]) + (p1[2] - p0[2]) * (p1[2] - p0[2]));
        float dist = sqrtf((p0[0] - c->root_center[0]) * (p0[0] - c->root_center[0]) + (p0[1] - c->root_center[1]) * (p0[1] - c->root_center[1]) +
                           (p0[2] - c->root_center[2]) * (p0[2] - c->root_center[2]));
        dist = dist < 0.05f * c->root_size ? 0.05f * c->root_size : dist;
        const float px = f_px * (ang > dp / dist ? ang : dp / dist);
        worst = !(px <= worst) ? px : worst;
    }
    return worst;
}

// Sky once can work at all: the option, the flags and lists (contexts with frames_per_launch >= 2), tiles of first_hit_kernel's size,
// the list's kernels in this program (kernels.h: launch_walk_list), and a call that goes at least TWICE round the ring.  The first
// ring's worth of frames and the launch that straddles the wrap go out full whatever happens, so in a shorter call the full frames
// outnumber the thin ones: it keeps the parent's launches throughout, and with them the bytes per frame that bench.py's model of the
// stage counts (48 B stored per pixel and frame; its counter passes over a short block are held against that model by
// test_bench_contract_line).  What that gives up is measured: HISTORY §17 (two thin launches of a 48-frame call's six, 2.7 %).
static bool sky_once_ready(const vxrt_ctx* c) {
    return c->sky_once != 0 && c->sky_tiles && !c->tile_sky.empty() && launch_walk_list != nullptr && c->call_frames >= 2u * c->ring.size();
}

// Everything a launch of g frames on stream `lane` will do, decided here and nowhere else, into p (all zero on entry).  Calls no HIP API and changes nothing: it
// reads the context as absorb_feedback left it (tail capacity, walking-tile count), the launch's cameras and the optional path poses.
static void plan_trace(TracePlan& p, const vxrt_ctx* c, uint32_t g, const Cam* cams, const CullBox& cull, const float (*path_pos)[3], const float (*path_dir)[3],
                       size_t lane, const int* slots, uint32_t gbuf_frames) {
    const bool wide = use_wide(c);
    const vxrt_ctx::TileSchedule& sched = c->schedules[lane];
    const bool ordered = c->use_tile_order && sched.valid;
    const unsigned tiles = trace_tile_count(c->band.width, c->band.local_rows);
    p.hbm = c->svo_count * sizeof(SvoRecord) + c->leaf_count * sizeof(int32_t) > kInfinityCacheBytes;
    // tracer 0 (auto) takes the all-in-one kernel (a) for scenes beyond the Infinity Cache (see auto_tracer) and (b) for ONE frame at
    // a time on one stream — the latency case of a render loop that calls vxrt_render per frame: the head + tail pair waits twice
    // for a longest wave (0.357 ms per 1080p bench frame), the single kernel once (0.267 ms); with frames in flight or several
    // frames per launch the pair wins (0.123 ms per frame at 16 x 2)
    p.tracer = (c->auto_tracer && (p.hbm || (g == 1 && c->inflight == 1))) ? 0 : c->trace_variant;
    p.wide_head = wide && (p.tracer == 0 || p.tracer == 4);
    p.wide_tail = wide;
    // when the tail is ONE launch its counters are copied back behind it (copy_counts); a tail that compacts again starts further launches
    p.single_tail_launch = p.tracer == 4;
    for (int k = c->tail_from + 1; p.single_tail_launch && k < int(c->cfg.max_bounces); k++)
        if (c->queues[lane].hitq[1] && ((c->tail_split >> k) & 1u)) p.single_tail_launch = false;
    // Fused head + tail (VXRT_OPT_FUSED_TAIL): one grid of persistent waves takes the launch's blocks and then its queued
    // paths, chunk by chunk as they become complete (trace.hip: fused_kernel).  For tails of ONE launch (the 4-bounce
    // benchmark; a tail that compacts again keeps its launches), the 8-byte records, scenes in cache.
    const bool fused = c->fused_tail && p.single_tail_launch && !wide && !p.hbm && c->tail_from < int(c->cfg.max_bounces);
    p.path = p.tracer == 0 ? TracePath::all_in_one : p.tracer == 2 ? TracePath::wavefront : p.tracer < 4 ? TracePath::ray_queue :
             fused ? TracePath::fused : p.tracer == 5 ? TracePath::head_paths : TracePath::head_bounces;
    const bool trace_kernel_head = p.path == TracePath::all_in_one || p.path == TracePath::head_bounces || p.path == TracePath::head_paths;
    // a wave of trace_kernel holds 8 (4) frames of one (two) rows of 8 pixels when the launch has whole groups of 8 (4) frames of ONE
    // camera — or of a slow camera path: at most 16 pixels across a group.  Not the wide records' kernel, nor the one for a scene in HBM:
    // those exist with one frame per wave only (trace.hip: launch_trace)
    p.frame_lanes = (c->frame_lanes && !wide && !p.hbm) ? (g % 8u == 0u ? 8 : (g % 4u == 0u ? 4 : 0)) : 0;
    if (p.frame_lanes && path_pos != nullptr && !(path_motion_px(c, g, uint32_t(p.frame_lanes), path_pos, path_dir) <= 16.0f)) p.frame_lanes = 0;
    // Shared primary rays (VXRT_OPT_SHARED_PRIMARY): when every frame of the launch has the camera of the first — decided by
    // comparing the cameras, not by who called — first_hit_kernel walks the band's primary rays once, ahead of trace_kernel on
    // this stream and inside the timed region, and trace_kernel's lanes load their pixel's record instead of casting.  Not for the
    // wide records, nor for a scene beyond the Infinity Cache (its kernel stays as measured: DESIGN.md section 5).
    p.share = trace_kernel_head && c->shared_primary && g >= 2 && lane < c->first_hits.size() && c->first_hits[lane] != nullptr && !wide && !p.hbm;
    for (uint32_t k = 1; p.share && k < g; k++) p.share = memcmp(&cams[k], &cams[0], sizeof(Cam)) == 0;
    // Option 1: the records belong to this launch alone.  Option 2: to the API call — a launch that shares walks only when no
    // earlier launch of this call has walked the same rays.  The records are a function of the camera, the cull state (a culled
    // lane writes no record, and trace_block reads one exactly when its own cull test fails: walker and reader must cull alike),
    // the band and the scene.  The first two are compared here; band and scene cannot change inside an API call, and the tag's call
    // id says the walk was this call's — nothing is kept from one call to the next, so no setter has to invalidate anything.
    p.walk = p.share;
    p.hits = lane;
    const vxrt_ctx::FirstHitTag& tag = c->first_hit_tag;
    if (p.share && c->shared_primary == 2 && tag.call != 0 && tag.call == c->call_id && tag.buffer < c->first_hits.size() &&
        memcmp(&tag.cam, &cams[0], sizeof(Cam)) == 0 && tag.cull == cull) {
        p.walk = false;
        p.hits = tag.buffer;
    }
    // (-DVXRT_VARIANTS=1 only: measured slower — the rest of the tiles are as chain-bound as the longest.)  The longest tiles apart
    // (VXRT_OPT_LONG_TILES, per mille of the tiles): the first tiles of the launch order — the longest chains of the last frames — run
    // as an all-in-one grid of their own on a second stream (fork_long_tiles), beside the head + tail pair of all other tiles.
    if (p.path == TracePath::head_bounces && c->long_tiles_permille > 0 && ordered && p.tracer == 4 && !wide && !p.hbm) {
        const unsigned n = unsigned((unsigned long long)tiles * c->long_tiles_permille / 1000u);
        p.long_blocks = (n < 1u ? 1u : (n >= tiles ? tiles - 1u : n)) * g;
    }
    // the priority split (issue_trace_kernel) needs the walking tiles first in the order and their number on the host
    if (trace_kernel_head && c->trace_priority && ordered && !sched.heavy_pending && p.long_blocks == 0u && sched.heavy < tiles) p.split_heavy = sched.heavy;
    // Sky once (VXRT_OPT_SKY_ONCE).  A tile none of whose pixels walks (first_hit_kernel: tile_sky) gets, from every block of
    // trace_kernel, values that depend on the camera, the cull box and the uniforms alone.  A full launch that shares under option 2
    // — the tag is this call's once it is issued, its frames have the tag's camera — leaves them in its slots (finish_launch: Slot::sky).
    // A later launch of the SAME call that reads the same records finds them there when every one of its slots says so, for its own
    // camera and cull box and with the G-buffer images where this launch wants them; it then goes out over the stream's list of the
    // tiles that walk alone (refresh_walk_list), when that list was cut from the tagged walk — and is not empty, which settle_thin
    // looks at.  The uniforms, the scene and the band cannot change inside a call, and a tag of another call matches nothing.
    // A walk notes the all-sky tiles when the pinned pair their numbers travel in is free (nearly always: see settle_thin).
    p.stamps_sky = sky_once_ready(c) && p.share && c->shared_primary == 2 && (p.walk ? !c->sky_count.pending : tag.sky);
    if (p.stamps_sky && !p.walk && p.long_blocks == 0u && p.split_heavy == 0u && lane < c->walk_lists.size()) {
        p.thin = c->walk_lists[lane].order_walk == tag.walk;
        for (uint32_t k = 0; p.thin && k < g; k++) {
            const vxrt_ctx::Slot::SkyTag& sky = c->ring[size_t(slots[k])].sky;
            p.thin = sky.call == c->call_id && memcmp(&sky.cam, &cams[0], sizeof(Cam)) == 0 && sky.cull == cull && (sky.gbuf || ((gbuf_frames >> k) & 1u) == 0u);
        }
    }
    // Re-sort the tiles for this stream's coming frames from the costs just measured: after its first
    // frame, then every 8th (costs keep accumulating as a running maximum in between; ~7 us per sort).
    if (batches_frames(p.tracer) && c->use_tile_order && (!sched.valid || sched.age >= 8))
        p.sort = (c->xcd_affinity > 0 && g == 1 && p.hbm) ? TileSort::xcd_affine : TileSort::longest_first;
}

// step 1: the cameras of the next g frames (path: optional poses, one per frame) and their frame slots: the next ones of the ring, never
// the temporal history
static void next_frames(vxrt_ctx* c, uint32_t g, int* slots, Cam* cams, Cam* olds, const float (*path_pos)[3], const float (*path_dir)[3]) {
    for (uint32_t k = 0; k < g; k++) {
        if (path_pos) {
            memcpy(c->cam_pos, path_pos[k], sizeof c->cam_pos);
            memcpy(c->cam_dir, path_dir[k], sizeof c->cam_dir);
        }
        update_bindings(c);
        cams[k] = c->cam;
        olds[k] = c->old_cam;
    }
    int s = c->slot;
    for (uint32_t k = 0; k < g; k++) {
        s = (s + 1) % int(c->ring.size());
        if (c->has_history && s == c->hist_slot) s = (s + 1) % int(c->ring.size());
        slots[k] = s;
    }
}

// step 2: the trace stream waits for whatever last used the slots
static int wait_for_slots(vxrt_ctx* c, uint32_t g, const int* slots, hipStream_t ts) {
    hipEvent_t waited = nullptr;
    for (uint32_t k = 0; k < g; k++) {   // the slots of an earlier launch share its event: wait for each event once
        vxrt_ctx::Slot& sl = c->ring[size_t(slots[k])];
        if (sl.last_use_recorded && sl.last_use != waited) {
            HIP_TRY(hipStreamWaitEvent(ts, sl.last_use, 0));
            waited = sl.last_use;
        }
    }
    return VXRT_OK;
}

// the pinned pair has arrived (its event has been seen)
static void take_sky_count(vxrt_ctx::SkyCount& sc) {
    sc.n_walk = sc.host[0];
    sc.skipped_pixels = sc.host[1];
    sc.walk = sc.pending_walk;
    sc.pending = false;
}

// step 3: what earlier launches of this stream reported, polled BEFORE the launch's timed region starts and before it is planned: the
// room its tail wanted (the queues grow: host wait + reallocation) and the number of walking tiles its last sort found
static int absorb_feedback(vxrt_ctx* c, size_t lane) {
    if (c->trace_variant >= 4 && !c->queues.empty()) { if (int rc = grow_tail_queues(c, lane)) return rc; }
    vxrt_ctx::TileSchedule& sched = c->schedules[lane];
    if (c->trace_priority && sched.heavy_pending && hipEventQuery(sched.heavy_ready) == hipSuccess) {
        sched.heavy = sched.host_heavy[0];
        sched.heavy_pending = false;
    }
    vxrt_ctx::SkyCount& sc = c->sky_count;   // the numbers of the last walk's all-sky tiles (issue_head)
    if (sc.pending && hipEventQuery(sc.ready) == hipSuccess) take_sky_count(sc);
    return VXRT_OK;
}

// step 4b (sky once): a launch that plan_trace found thin needs the walk's numbers.  They left right behind first_hit_kernel in the
// call's first launch, and no launch can be thin before the call has been once around the ring: they are here, unless the host has
// run that far ahead of the GPU — then it waits for them, with at least the ring's worth of launches queued behind that event.  An
// all-sky view keeps the full launch: block 0 of trace_kernel rotates the tail's counters (zero_counts), so there must be one.
static int settle_thin(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    vxrt_ctx::SkyCount& sc = c->sky_count;
    const uint64_t walk = c->first_hit_tag.walk;
    if (sc.pending && sc.pending_walk == walk) {
        HIP_TRY(hipEventSynchronize(sc.ready));
        take_sky_count(sc);
    }
    L.plan.thin = sc.walk == walk && sc.n_walk > 0u && sc.n_walk <= trace_tile_count(c->band.width, c->band.local_rows);
    if (L.plan.thin) { L.plan.n_walk = sc.n_walk; L.plan.skipped_pixels = sc.skipped_pixels; }
    return VXRT_OK;
}

// step 5: the kernels' arguments for the planned launch
static void fill_trace_args(TraceLaunch& L, const Cam* cams, uint32_t gbuf_frames, uint32_t first_frame_number) {
    const vxrt_ctx* c = L.c;
    TraceArgs& a = L.a;
    const uint32_t g = L.g;
    const vxrt_ctx::TileSchedule& sched = c->schedules[L.lane];
    frame_constants(c, a);
    for (uint32_t k = 0; k < g; k++) {
        const vxrt_ctx::Slot& sl = c->ring[size_t(L.slots[k])];
        a.out[k] = FrameOut{sl.sampled_color, sl.nd, sl.albedo};
        a.cams[k] = cams[k];
    }
    a.out_color = a.out[0].color; a.out_nd = a.out[0].nd; a.out_albedo = a.out[0].albedo;
    a.batch = int(g);
    a.gbuf_frames = gbuf_frames;
    a.frame_lanes = L.plan.frame_lanes;
    set_cull(a, L.cull);
    a.ray_counter = c->d_rays;
    a.tile_order = (c->use_tile_order && sched.valid) ? sched.order : nullptr;
    a.tile_cost = c->use_tile_order ? sched.cost : nullptr;
    a.frame_number = first_frame_number;
    a.cam = cams[0];
    a.tail = PathQueue{nullptr, nullptr, 0};
    a.tail_zero = nullptr;
    a.tail_from = 0;
    if (L.plan.tracer != 0) L.counts = CountSets(c->queues[L.lane]);
    if (L.plan.tracer >= 4) {   // the head hands its live paths over: to the set this launch writes, clearing the next launch's
        a.tail = PathQueue{c->queues[L.lane].hitq[0], L.counts.written(), c->shard_capacity};
        a.tail_zero = L.counts.cleared();
        a.tail_from = c->tail_from;
    }
}

// How much room this launch wanted: its counter set (and, for fused_kernel, its error word: `also`), copied back for grow_tail_queues;
// skipped while an earlier copy is pending.  The set stays untouched until launch J + 2 clears it, so when the tail is ONE launch
// (J + 1) the copy goes behind it — a copy between the head and the tail costs the stream ~10 us of copy-engine hand-over on a block's
// critical path (round 5: the time line of a rank of 8 showed trace_kernel -> 4 us copy -> 5.6 us gap -> bounce_kernel); a tail of
// several launches clears it sooner
static int copy_counts(vxrt_ctx* c, vxrt_ctx::StreamQueues& sq, const unsigned* written, hipStream_t ts, void* also_to = nullptr, const void* also_from = nullptr) {
    if (sq.counts_pending) return VXRT_OK;
    HIP_TRY(hipMemcpyAsync(sq.host_counts, written, 64 * 64, hipMemcpyDeviceToHost, ts));
    if (also_to) HIP_TRY(hipMemcpyAsync(also_to, also_from, 4, hipMemcpyDeviceToHost, ts));
    HIP_TRY(hipEventRecord(sq.counts_ready, ts));
    sq.counts_pending = true;
    sq.counts_capacity = c->shard_capacity;
    return VXRT_OK;
}

// One launch of trace_kernel over the launch's tiles from block plan.long_blocks on — or, with VXRT_OPT_TRACE_PRIORITY and a tile order
// whose walking tiles are known, as TWO grids: the tiles that walk (the first `split_heavy` of the plain longest-first order) on the
// high-priority trace stream, the tiles that only store sky on the lane's low-priority stream, forked and joined by events, so that
// the dispatcher takes blocks of the long chains first whenever both grids have blocks waiting.  Same blocks, same arithmetic.
static int issue_trace_kernel(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    const TracePlan& p = L.plan;
    if (p.thin) {   // the tiles that walk alone, in the launch order's sequence; the others hold their sky (plan_trace)
        const uint32_t* whole = L.a.tile_order;
        L.a.tile_order = c->walk_lists[L.lane].order;
        const hipError_t e = launch_trace(L.a, p.wide_head, p.hbm, L.ts, 0u, p.n_walk * L.g);
        L.a.tile_order = whole;
        HIP_TRY(e);
        return VXRT_OK;
    }
    if (p.split_heavy == 0u) {
        HIP_TRY(launch_trace(L.a, p.wide_head, p.hbm, L.ts, p.long_blocks, 0u));
        return VXRT_OK;
    }
    HIP_TRY(hipEventRecord(c->low_fork[L.lane], L.ts));                         // after everything this launch waits for
    HIP_TRY(hipStreamWaitEvent(c->low_streams[L.lane], c->low_fork[L.lane], 0));
    HIP_TRY(launch_trace(L.a, p.wide_head, p.hbm, L.ts, 0u, p.split_heavy * L.g));                        // high priority: the chains
    HIP_TRY(launch_trace(L.a, p.wide_head, p.hbm, c->low_streams[L.lane], p.split_heavy * L.g, 0u));      // low priority: the stores
    HIP_TRY(hipEventRecord(c->low_join[L.lane], c->low_streams[L.lane]));
    return VXRT_OK;
}

// The longest tiles as an all-in-one grid of their own on the lane's second stream (no hand-over: a path's whole chain in ONE wave,
// begun at the launch's start).  A launch that is little more than its chains (a rank's share of a short block on 8 GPUs) is two
// chains long as head + tail and one as the all-in-one kernel, which in turn needs 1.3 x the instructions: this takes the one chain
// where it matters and the cheaper instructions everywhere else.  Same pixels, same arithmetic, either way.
static int fork_long_tiles(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    const size_t lane = L.lane;
    if (c->aux_streams.size() <= lane) c->aux_streams.resize(lane + 1);
    if (c->aux_fork.size() <= lane) { c->aux_fork.resize(lane + 1); c->aux_join.resize(lane + 1); }
    if (c->aux_join[lane] == nullptr) {   // made last: all three are there
        HIP_TRY(c->aux_streams[lane].create(hipStreamNonBlocking));
        HIP_TRY(c->aux_fork[lane].create(hipEventDisableTiming));
        HIP_TRY(c->aux_join[lane].create(hipEventDisableTiming));
    }
    TraceArgs al = L.a;
    al.tail = PathQueue{nullptr, nullptr, 0};     // nothing is handed over: trace_kernel follows these paths to their end
    al.tail_zero = nullptr;
    HIP_TRY(hipEventRecord(c->aux_fork[lane], L.ts));                       // after everything this launch waits for
    HIP_TRY(hipStreamWaitEvent(c->aux_streams[lane], c->aux_fork[lane], 0));
    HIP_TRY(launch_trace(al, false, false, c->aux_streams[lane], 0u, L.plan.long_blocks));
    HIP_TRY(hipEventRecord(c->aux_join[lane], c->aux_streams[lane]));
    return VXRT_OK;
}

// Sky once: the launch's stream gets its order (as the stream's next launch will take it) without the all-sky tiles of the tagged walk
static int cut_walk_list(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    const vxrt_ctx::FirstHitTag& tag = c->first_hit_tag;
    vxrt_ctx::WalkList& wl = c->walk_lists[L.lane];
    const vxrt_ctx::TileSchedule& sched = c->schedules[L.lane];
    HIP_TRY(launch_walk_list((c->use_tile_order && sched.valid) ? sched.order.get() : nullptr, c->tile_sky[tag.buffer], c->use_tile_order ? sched.cost.get() : nullptr,
                             wl.order, wl.partial, trace_tile_count(c->band.width, c->band.local_rows), L.ts));
    wl.order_walk = tag.walk;
    return VXRT_OK;
}

// The all-in-one launch, and the head of a head + tail pair: the long tiles' grid (its arguments are copied before the first hits are
// set: it casts its own), the first hits when the launch shares its primary rays — its own walk or an earlier one's — trace_kernel.
static int issue_head(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    if (L.plan.long_blocks != 0u) { if (int rc = fork_long_tiles(L)) return rc; }
    if (L.plan.share) {
        const size_t b = L.plan.hits, streams = c->trace_streams.size();
        vxrt_ctx::FirstHitTag& tag = c->first_hit_tag;
        L.a.first_hit = c->first_hits[b];
        if (L.plan.walk) {
            if (L.plan.stamps_sky && c->shared_primary == 2 && b < c->tile_sky.size() && L.lane < c->walk_lists.size())
                L.a.tile_sky = c->tile_sky[b];   // the walk notes the all-sky tiles as well
            // The walk overwrites buffer b (b == this stream).  Who may still be reading it?  Launches of this stream are over
            // before the walk starts: the stream's order.  A launch of another stream s that read b noted its event in
            // first_hit_readers (finish_launch), and launches of s are ordered among themselves, so waiting for the LAST reader on
            // each s covers all of them.  Those events were recorded before this call to hipStreamWaitEvent, by this thread: the
            // wait cannot refer to work not yet issued, and it costs the host nothing.  (A launch_events entry is recorded again two
            // launches later on its stream; the wait then covers that later launch as well — more than needed, never less.)
            for (size_t s = 0; s < streams; s++) {
                hipEvent_t& reader = c->first_hit_readers[b * streams + s];
                if (reader != nullptr && s != L.lane) HIP_TRY(hipStreamWaitEvent(L.ts, reader, 0));
                reader = nullptr;
            }
            tag.call = 0;   // the tagged records are overwritten now, or are superseded below, or were another call's
            HIP_TRY(launch_first_hit(L.a, L.ts));
            if (c->shared_primary == 2) {
                HIP_TRY(hipEventRecord(c->first_hit_walked[b], L.ts));
                tag.call = c->call_id;
                tag.buffer = b;
                tag.cam = L.a.cams[0];
                tag.cull = L.cull;
                tag.walk = ++c->walk_serial;
                tag.sky = L.a.tile_sky != nullptr;
                // Sky once: this stream's list right away — a few microseconds ahead of trace_kernel, once per call — because its
                // numbers are the walk's, and the host wants them when the call comes back to its first ring slot (settle_thin)
                if (tag.sky) {
                    vxrt_ctx::SkyCount& sc = c->sky_count;
                    if (int rc = cut_walk_list(L)) return rc;
                    HIP_TRY(hipMemcpyAsync(sc.host, c->walk_lists[L.lane].partial + 2 * kSortBlocks, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, L.ts));
                    HIP_TRY(hipEventRecord(sc.ready, L.ts));
                    sc.pending = true;
                    sc.pending_walk = tag.walk;
                }
            }
        } else if (b != L.lane) {
            HIP_TRY(hipStreamWaitEvent(L.ts, c->first_hit_walked[b], 0));   // the walker's own stream needs no wait
        }
    }
    return issue_trace_kernel(L);
}

// the tail as launches of bounce_kernel; without a second queue (tail_split == 0) nothing is appended to queues[1]: its capacity 0 says so
static int tail_bounces(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    vxrt_ctx::StreamQueues& sq = c->queues[L.lane];
    PathQueue queues[2] = {{sq.hitq[0], nullptr, c->shard_capacity}, {sq.hitq[1], nullptr, sq.hitq[1] ? c->shard_capacity : 0u}};
    HIP_TRY(launch_bounces(L.a, L.plan.wide_tail, queues, L.counts.sets, &sq.launches, c->trace_blocks, sq.hitq[1] ? c->tail_split : 0u, c->tail_from, L.ts));
    return VXRT_OK;
}

#if VXRT_VARIANTS
// the tail as one launch of path_kernel, which reads the set the head wrote and clears the one launch J read
static int tail_paths(TraceLaunch& L) {
    HIP_TRY(launch_paths(L.a, L.a.tail, L.counts.read(), L.c->tail_from, L.c->path_blocks, L.ts));
    L.c->queues[L.lane].launches = L.counts.J + 2;
    return VXRT_OK;
}
#endif

// head + tail: trace_kernel hands the paths alive at hit tail_from to `tail`
static int issue_head_tail(TraceLaunch& L, int (*tail)(TraceLaunch&)) {
    vxrt_ctx* c = L.c;
    vxrt_ctx::StreamQueues& sq = c->queues[L.lane];
    const CountSets& counts = L.counts;
    if (int rc = issue_head(L)) return rc;
    if (c->head_stagger) {
        HIP_TRY(hipEventRecord(c->head_events[L.lane], L.ts));
        c->last_head_lane = int(L.lane);
    }
    sq.launches = counts.J + 1;
    if (!L.plan.single_tail_launch) { if (int rc = copy_counts(c, sq, counts.written(), L.ts)) return rc; }
    if (int rc = tail(L)) return rc;
    if (L.plan.single_tail_launch) { if (int rc = copy_counts(c, sq, counts.written(), L.ts)) return rc; }
    if (L.plan.long_blocks != 0u) HIP_TRY(hipStreamWaitEvent(L.ts, c->aux_join[L.lane], 0));   // the launch is over when both grids are
    return VXRT_OK;
}

#if VXRT_VARIANTS
// head and tail as ONE grid of persistent waves (plan_trace: fused).  It wrote set (J + 1) % 3 and cleared (J + 2) % 3, which the next launch writes.
static int issue_fused(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    vxrt_ctx::StreamQueues& sq = c->queues[L.lane];
    const CountSets& counts = L.counts;
    if (sq.host_ctl == nullptr) {   // made last: both are there
        HIP_TRY(sq.fused_ctl.alloc(fused_ctl_bytes()));
        HIP_TRY(sq.host_ctl.alloc(64 / sizeof(unsigned)));    // word 2: the kernel's error word
        memset(sq.host_ctl, 0, 64);
    }
    if (!sq.stamps_clean) {   // once per allocation of the queue: every slot's stamp must read 0
        HIP_TRY(hipMemsetAsync(sq.hitq[0], 0, (size_t(c->shard_capacity) * 64 + 1) * 64, L.ts));
        sq.stamps_clean = true;
    }
    HIP_TRY(hipMemsetAsync(sq.fused_ctl, 0, fused_ctl_bytes(), L.ts));
    const uint32_t stamp = (sq.fused_launches++ % 65535u) + 1u;
    const unsigned all_blocks = trace_tile_count(c->band.width, c->band.local_rows) * L.g;
    const unsigned fused_slots = c->wave_slots / 5u * 4u;      // fused_kernel is compiled for 4 waves per SIMD (trace.hip: VXRT_FUSED_WAVES)
    HIP_TRY(launch_fused(L.a, sq.fused_ctl, fused_slots < all_blocks ? fused_slots : all_blocks, L.a.tile_order ? c->schedules[L.lane].scratch : nullptr, stamp, L.ts));
    sq.launches = counts.J + 1;
    return copy_counts(c, sq, counts.written(), L.ts, sq.host_ctl + 2, sq.fused_ctl + fused_ctl_error_offset());
}

// tracers 2 and 3: the launches per path segment of the wavefront and of the ray queues
static int issue_queued(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    vxrt_ctx::StreamQueues& sq = c->queues[L.lane];
    PathQueue queues[2] = {{sq.hitq[0], nullptr, c->shard_capacity}, {sq.hitq[1], nullptr, c->shard_capacity}};
    CountSets& counts = L.counts;
    if (L.plan.path == TracePath::wavefront)
        HIP_TRY(launch_trace_wavefront(L.a, queues, counts.sets, &sq.launches, c->trace_blocks, c->trace_split, L.ts));
    else
        HIP_TRY(launch_trace_rayqueue(L.a, queues[0], counts.sets, &sq.launches, sq.rq, c->shade_blocks, c->trace_blocks, c->rays_per_wave, L.ts));
    return VXRT_OK;
}
#endif

// step 6: the planned path's launches.  Head stagger (VXRT_OPT_HEAD_STAGGER): the head of a head + tail launch starts when the previous
// launch's head (another stream) has finished, so that a head runs beside the previous launch's tail instead of beside its head
static int issue(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    if (L.plan.tracer >= 4 && c->head_stagger && c->last_head_lane >= 0 && size_t(c->last_head_lane) != L.lane)
        HIP_TRY(hipStreamWaitEvent(L.ts, c->head_events[size_t(c->last_head_lane)], 0));
    switch (L.plan.path) {
        case TracePath::all_in_one: return issue_head(L);
        case TracePath::head_bounces: return issue_head_tail(L, tail_bounces);
#if VXRT_VARIANTS
        case TracePath::head_paths: return issue_head_tail(L, tail_paths);
        case TracePath::fused: return issue_fused(L);
        case TracePath::wavefront:
        case TracePath::ray_queue: return issue_queued(L);
#endif
        default: return VXRT_OK;   // a tracer this build does not hold: vxrt_create refuses it
    }
}

// step 7: the stream's tile order for its coming frames (plan_trace: sort), after the timed region
static int resort_tiles(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    const TileSort sort = L.plan.sort;
    hipStream_t ts = L.ts;
    vxrt_ctx::TileSchedule& sched = c->schedules[L.lane];
    if (!batches_frames(L.plan.tracer)) return VXRT_OK;   // the queue-based tracers take their tiles in raster order
    if (sort == TileSort::xcd_affine) {
        if (int rc = xcd_affine_order(c, sched, ts)) return rc;
    } else if (sort == TileSort::longest_first) {
        // (the priority split needs the walking tiles FIRST in the order: no spreading; and their number on the host)
        HIP_TRY(launch_tile_order(sched.cost, sched.order, sched.last_cost, sched.scratch, trace_tile_count(c->band.width, c->band.local_rows),
                                  L.g * unsigned(c->inflight), c->wave_slots, c->trace_priority ? 0 : c->spread_override, ts));
        if (c->trace_priority) {
            if (sched.heavy_pending) HIP_TRY(hipEventSynchronize(sched.heavy_ready));
            HIP_TRY(hipMemcpyAsync(sched.host_heavy, sched.scratch + 128 * 64, sizeof(unsigned), hipMemcpyDeviceToHost, ts));
            HIP_TRY(hipEventRecord(sched.heavy_ready, ts));
            sched.heavy_pending = true;
        }
    }
    if (sort != TileSort::none) { sched.valid = true; sched.age = 0; }
    sched.age++;
    return VXRT_OK;
}

// step 7b (sky once): the stream's launch order without the all-sky tiles, cut again whenever the tagged walk or the order is new —
// behind the timed region, on the launch's stream: the next launch of the stream finds it by the stream's order.  The flags are read
// from the tagged buffer, which this launch's kernels read as well: the next walk into that buffer waits for this launch's event
// (finish_launch: first_hit_readers), recorded behind the list.  A re-sort changes the order, not the numbers: nothing travels.
static int refresh_walk_list(TraceLaunch& L) {
    vxrt_ctx* c = L.c;
    if (L.lane >= c->walk_lists.size()) return VXRT_OK;
    vxrt_ctx::WalkList& wl = c->walk_lists[L.lane];
    if (L.plan.sort != TileSort::none) wl.order_walk = 0;   // the order it was cut from is gone
    const vxrt_ctx::FirstHitTag& tag = c->first_hit_tag;
    if (!L.plan.stamps_sky || tag.call != c->call_id || !tag.sky || wl.order_walk == tag.walk) return VXRT_OK;
    return cut_walk_list(L);
}

// step 8: one event for the whole launch, the slots' and the context's books, and the three counters of what went out
static int finish_launch(TraceLaunch& L, bool timed) {
    vxrt_ctx* c = L.c;
    const size_t lane = L.lane;
    const uint32_t g = L.g;
    hipEvent_t done = c->launch_events[lane * 2 + (c->launch_event_turn[lane]++ & 1u)];
    HIP_TRY(hipEventRecord(done, L.ts));
    for (uint32_t k = 0; k < g; k++) {
        vxrt_ctx::Slot& sl = c->ring[size_t(L.slots[k])];
        sl.trace_done = done;
        sl.last_use = done;              // until a later stage reads the slot, the trace is its last use
        sl.last_use_recorded = true;
        // what the slot's all-sky tiles hold now: a thin launch left them alone; a full one stored this call's sky, or something else
        if (L.plan.thin) continue;
        sl.sky.call = 0;
        if (L.plan.stamps_sky) {
            sl.sky.call = c->call_id;
            sl.sky.cam = L.a.cams[0];
            sl.sky.cull = L.cull;
            sl.sky.gbuf = ((L.a.gbuf_frames >> k) & 1u) != 0u;
        }
    }
    c->slot = L.slots[g - 1];
    c->last_schedule = int(lane);
    c->trace_launches += 1;
    c->traced += g;
    c->frames += g;
    c->pixels += uint64_t(g) * uint64_t(c->band.local_rows) * c->band.width;
    if (timed) { c->timed_frames += g; c->timed_launches += 1; }
    c->accum_is_sampled = true;
    c->halo_valid = false;
    if (L.plan.frame_lanes) c->frame_lane_launches++;
    if (L.plan.share) {
        c->shared_primary_launches++;
        c->first_hit_readers[L.plan.hits * c->trace_streams.size() + lane] = done;   // issue_head: the next walk into that buffer waits for it
    }
    if (L.plan.walk) c->first_hit_walks++;
    if (L.plan.split_heavy) c->split_launches++;
    if (c->band.local_rows > 0 && (L.plan.path == TracePath::all_in_one || L.plan.path == TracePath::head_bounces || L.plan.path == TracePath::head_paths))
        c->trace_kernel_blocks += uint64_t(L.plan.thin ? L.plan.n_walk : trace_tile_count(c->band.width, c->band.local_rows)) * g;
    if (L.plan.thin) {
        c->thin_launches++;
        c->sky_rays += uint64_t(g) * L.plan.skipped_pixels;   // one cast_bounded_ray per pixel and frame, as a culled lane counts it (trace_block)
    }
    return VXRT_OK;
}

// The trace stage of the next g frames (parameters at rest) as ONE launch of the tracer: g ring slots, frame numbers
// frame_number+1 .. +g.  g > 1 only with the tracers that take several frames per launch (ctx.h: batches_frames).  slots[k] = ring slot
// of frame k.  path: optional g camera poses (position, direction), one per frame; null = the camera stays where it is.  cams / olds
// (g entries each): the camera and the "old" camera of every frame, as temporal.comp and denoise.comp of that frame see them.
// The steps: cameras and slots, waits, feedback of earlier launches, the plan, the kernels' arguments, the planned path's launches
// between the timed pair's events, the tile re-sort, the books.  A rank without rows launches nothing and plans nothing.
int trace_frames(vxrt_ctx* c, uint32_t g, bool timed, int* slots, Cam* cams, Cam* olds, const float (*path_pos)[3], const float (*path_dir)[3],
                 uint32_t gbuf_frames) {
    const uint32_t first_frame_number = c->uniforms.frame_number + 1;
    next_frames(c, g, slots, cams, olds, path_pos, path_dir);
    const size_t lane = size_t(c->trace_launches % uint64_t(c->inflight));
    hipStream_t ts = c->trace_streams[lane];
    if (int rc = wait_for_slots(c, g, slots, ts)) return rc;
    TraceLaunch L(c, ts, lane, g, slots);
    if (c->band.local_rows > 0) {
        if (int rc = absorb_feedback(c, lane)) return rc;
        L.cull = cull_box(c, cams, g);
        plan_trace(L.plan, c, g, cams, L.cull, path_pos, path_dir, lane, slots, gbuf_frames);
        if (L.plan.thin) { if (int rc = settle_thin(L)) return rc; }
        fill_trace_args(L, cams, gbuf_frames, first_frame_number);
        EventPair p;
        if (timed) { p = take_pair(c, 0); HIP_TRY(hipEventRecord(p.a, ts)); }
        if (int rc = issue(L)) return rc;
        // the launch is over when both grids of a priority split are (a no-op before the first split)
        if (c->trace_priority && batches_frames(L.plan.tracer)) HIP_TRY(hipStreamWaitEvent(ts, c->low_join[lane], 0));
        if (timed) HIP_TRY(hipEventRecord(p.b, ts));
        if (int rc = resort_tiles(L)) return rc;
        if (int rc = refresh_walk_list(L)) return rc;
        if (timed) c->pending.push_back(p);
    }
    return finish_launch(L, timed);
}

}  // namespace vxrt
