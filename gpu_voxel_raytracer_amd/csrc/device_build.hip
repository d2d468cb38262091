// device_build.hip — the octree of an arbitrary voxel list built on the device (vxrt_device_scene.h), straight into the records the
// tracers read: byte for byte what flatten_svo(build_octree(list)) makes on the host (api_scene.hip, scene_host.cpp).
//
// The host layout, restated without pointers.  With d the depth and u = p + 2^d per axis, a voxel's path key interleaves u's bits,
// x highest: key = sum over k = 0 .. d of (bit k of u.x << 2 | bit k of u.y << 1 | bit k of u.z) << 3k (vxrt_extract.h).  The
// records are breadth first, so level-major, and within a level in ascending path key.  The node of level d - j + 1 that holds a
// voxel is key >> 3j (j = 1: the leaf parents; j = d + 1: the root); its slot for the voxel is (key >> 3(j - 1)) & 7.  A leaf
// parent's base is the index of its first leaf word; the leaf words are in ascending key order.  An inner node's base is the index
// of its first child.  The last entry for a position wins.
//
// Pipeline (every step its own launch; every position a prefix sum in input order; nothing waits on another workgroup):
//   bounds        block min / max of every coordinate, then one workgroup over the blocks -> 8 bytes read back: the depth
//   keys          per entry: the path key (<= 48 bits) and the leaf word
//   radix sort    stable LSD over the 3(d + 1) key bits, 8 bits per pass; a pass is hist (block digit counts, digit-major),
//                 scan (one workgroup per digit over the blocks), scatter (rank in the block by wave ballots + LDS, stage the block
//                 sorted in LDS, write runs of one digit contiguously)
//   dedupe        the last entry of every run of equal keys, compacted by a scan: its leaf word is d_leaves, its key the unique list
//                 (radix sort and dedupe are sort_unique_list, which vxrt_edit_voxels_device runs at a loaded scene's depth)
//   level counts  per unique key, the number of levels at which it opens a node (from the highest bit in which it differs from
//                 its predecessor) -> every level's node count -> the exact record count, one allocation
//   levels        bottom-up, per level: count / scan / write the runs of key >> 3 of the level below (each run at most 8 long):
//                 its mask, its base, and its key for the level above, written at the level's final (top-down) position.
#include <climits>
#include <string>

#include "block_scan.h"
#include "ctx.h"
#include "device_build.h"

namespace vxrt {
namespace {

constexpr uint32_t kThreads = 256;                  // every kernel but the scans (kThreads == kDigits: one thread per digit)
constexpr uint32_t kWaves = kThreads / 64;
constexpr uint32_t kItems = 16;                     // entries per thread
constexpr uint32_t kTile = kThreads * kItems;       // entries per block: 4096
constexpr uint32_t kDigits = 256;
constexpr uint32_t kRowThreads = 1024;              // radix_scan: one workgroup per digit
constexpr uint32_t kBoundsBlocks = 1024;
constexpr uint32_t kLevelBins = 17;                 // a unique key opens nodes at levels 1 .. t, t = 0 .. 16
constexpr uint32_t kScanThreads = 1024;             // exclusive_scan: one workgroup, 8 partials per thread per pass
constexpr uint32_t kScanItems = 8;

uint32_t tiles(size_t n) { return uint32_t((n + kTile - 1) / kTile); }

// the lanes of this wave that are valid and hold the same 8-bit digit as this lane
__device__ __forceinline__ uint64_t digit_peers(uint32_t d, bool ok) {
    uint64_t peers = __ballot(ok);
#pragma unroll
    for (uint32_t b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t m = __ballot(bit);
        peers &= bit ? m : ~m;
    }
    return peers;
}

// ---- bounds --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void min_max8(uint4 w, int* lo, int* hi) {
    const uint32_t q[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int a = int(int16_t(q[k] & 0xffffu)), b = int(int16_t(q[k] >> 16));
        *lo = min(*lo, min(a, b));
        *hi = max(*hi, max(a, b));
    }
}

__device__ __forceinline__ void block_min_max(int lo, int hi, int2* out) {
    __shared__ int s_lo[kWaves], s_hi[kWaves];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63u) == 0u) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < kWaves; w++) { lo = min(lo, s_lo[w]); hi = max(hi, s_hi[w]); }
        *out = make_int2(lo, hi);
    }
}

// count int16 values (3 per voxel); vec: pos is 16-byte aligned, so the first count / 8 * 8 values are read 8 at a time
__global__ __launch_bounds__(kThreads) void bounds_kernel(const int16_t* pos, size_t count, uint32_t vec, int2* part) {
    int lo = INT_MAX, hi = INT_MIN;
    const size_t stride = size_t(gridDim.x) * kThreads;
    size_t i = size_t(blockIdx.x) * kThreads + threadIdx.x;
    size_t tail = 0;
    if (vec) {
        const uint4* w = reinterpret_cast<const uint4*>(pos);
        const size_t n8 = count / 8;
        for (size_t k = i; k < n8; k += stride) min_max8(w[k], &lo, &hi);
        tail = n8 * 8;
    }
    for (size_t k = tail + i; k < count; k += stride) { lo = min(lo, int(pos[k])); hi = max(hi, int(pos[k])); }
    block_min_max(lo, hi, part + blockIdx.x);
}

__global__ __launch_bounds__(kThreads) void bounds_reduce_kernel(int2* part, uint32_t blocks) {
    int lo = INT_MAX, hi = INT_MIN;
    for (uint32_t k = threadIdx.x; k < blocks; k += kThreads) { lo = min(lo, part[k].x); hi = max(hi, part[k].y); }
    block_min_max(lo, hi, part + blocks);
}

// ---- keys ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void keys_kernel(const int16_t* pos, const uint8_t* mrgb, size_t n, uint32_t depth, uint32_t words,
                                                         uint64_t* keys, uint32_t* vals) {
    const size_t i = size_t(blockIdx.x) * kThreads + threadIdx.x;
    if (i >= n) return;
    const int half = 1 << depth;
    const uint32_t ux = uint32_t(int(pos[3 * i + 0]) + half), uy = uint32_t(int(pos[3 * i + 1]) + half), uz = uint32_t(int(pos[3 * i + 2]) + half);
    uint32_t m, r, g, b;
    if (words) {
        const uint32_t w = reinterpret_cast<const uint32_t*>(mrgb)[i];
        m = w & 0xffu; r = (w >> 8) & 0xffu; g = (w >> 16) & 0xffu; b = w >> 24;
    } else {
        m = mrgb[4 * i + 0]; r = mrgb[4 * i + 1]; g = mrgb[4 * i + 2]; b = mrgb[4 * i + 3];
    }
    keys[i] = path_key_of(ux, uy, uz, depth);
    vals[i] = leaf_word_of(m, r, g, b);
}

// ---- radix sort ----------------------------------------------------------------------------------------------------------------
// hist[digit * blocks + block]: the block's count of the digit
__global__ __launch_bounds__(kThreads) void radix_hist_kernel(const uint64_t* keys, uint32_t n, uint32_t shift, uint32_t blocks, uint32_t* hist) {
    __shared__ uint32_t cnt[kDigits];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t base = size_t(blockIdx.x) * kTile;
#pragma unroll 4
    for (uint32_t j = 0; j < kItems; j++) {
        const size_t i = base + j * kThreads + threadIdx.x;
        const bool ok = i < n;
        const uint32_t d = ok ? uint32_t(keys[i] >> shift) & 0xffu : 0u;
        const uint64_t peers = digit_peers(d, ok);
        if (ok && lanes_below(peers) == 0u) atomicAdd(&cnt[d], uint32_t(__popcll(peers)));   // LDS: one add per digit per wave
    }
    __syncthreads();
    hist[size_t(threadIdx.x) * blocks + blockIdx.x] = cnt[threadIdx.x];
}

// one workgroup per digit: its row of hist -> exclusive prefix sums in place; totals[digit] = the row's sum
__global__ __launch_bounds__(kRowThreads) void radix_scan_kernel(uint32_t* hist, uint32_t blocks, uint32_t* totals) {
    __shared__ uint32_t lds[kRowThreads / 64];
    uint32_t* row = hist + size_t(blockIdx.x) * blocks;
    uint32_t carry = 0;
    for (uint32_t c = 0; c < blocks; c += kRowThreads) {
        const uint32_t i = c + threadIdx.x;
        const uint32_t v = i < blocks ? row[i] : 0u;
        uint32_t total;
        const uint32_t o = carry + block_exclusive<uint32_t, kRowThreads / 64>(v, lds, &total);
        if (i < blocks) row[i] = o;
        carry += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = carry;
}

// Stable: the tile's entries are ranked in input order (round j, then wave, then lane), staged digit-sorted in LDS and written out
// so that each digit's entries of the tile form one contiguous run at hist's offset.
// kVals: the keys carry values (a clear list of vxrt_edit_voxels_device has none: vals_in / vals_out are null and never touched).
template <bool kVals>
__global__ __launch_bounds__(kThreads) void radix_scatter_kernel(const uint64_t* keys_in, const uint32_t* vals_in, uint64_t* keys_out,
                                                                 uint32_t* vals_out, uint32_t n, uint32_t shift, uint32_t blocks,
                                                                 const uint32_t* hist, const uint32_t* totals) {
    __shared__ uint64_t s_key[kTile];
    __shared__ uint32_t s_val[kVals ? kTile : 1];
    __shared__ uint32_t s_wave[2][kWaves][kDigits];   // per round (double-buffered): entries of a digit per wave -> their offsets
    __shared__ uint32_t s_start[kDigits];             // a digit's first entry in the staged tile
    __shared__ uint32_t s_dst[kDigits];               // ... and in the output
    __shared__ uint32_t s_scan[kWaves];
    const uint32_t t = threadIdx.x, wave = t >> 6;
    const size_t base = size_t(blockIdx.x) * kTile;
    uint64_t key[kItems];
    uint32_t val[kVals ? kItems : 1], rank[kItems];
#pragma unroll
    for (uint32_t w = 0; w < kWaves; w++) s_wave[0][w][t] = 0u;
    __syncthreads();
    uint32_t run = 0;   // thread t: entries of digit t in the rounds so far
#pragma unroll
    for (uint32_t j = 0; j < kItems; j++) {
        const uint32_t b = j & 1u;
        const size_t i = base + j * kThreads + t;
        const bool ok = i < n;
        key[j] = ok ? keys_in[i] : 0ull;
        if (kVals) val[j] = ok ? vals_in[i] : 0u;
        const uint32_t d = uint32_t(key[j] >> shift) & 0xffu;
        const uint64_t peers = digit_peers(d, ok);
        const uint32_t below = lanes_below(peers);
        if (ok && below == 0u) s_wave[b][wave][d] = uint32_t(__popcll(peers));
        __syncthreads();
        uint32_t acc = run;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; w++) {
            const uint32_t c = s_wave[b][w][t];
            s_wave[b][w][t] = acc;
            s_wave[b ^ 1u][w][t] = 0u;   // the next round's counters (last read before this round's first barrier)
            acc += c;
        }
        run = acc;
        __syncthreads();
        rank[j] = s_wave[b][wave][d] + below;
    }
    uint32_t total;
    s_start[t] = block_exclusive<uint32_t, kWaves>(run, s_scan, &total);
    s_dst[t] = block_exclusive<uint32_t, kWaves>(totals[t], s_scan, &total) + hist[size_t(t) * blocks + blockIdx.x];
#pragma unroll
    for (uint32_t j = 0; j < kItems; j++) {
        if (base + j * kThreads + t < n) {
            const uint32_t p = s_start[uint32_t(key[j] >> shift) & 0xffu] + rank[j];
            s_key[p] = key[j];
            if (kVals) s_val[p] = val[j];
        }
    }
    __syncthreads();
    const uint32_t count = uint32_t(min(size_t(kTile), size_t(n) - base));
    for (uint32_t p = t; p < count; p += kThreads) {
        const uint64_t k = s_key[p];
        const uint32_t d = uint32_t(k >> shift) & 0xffu;
        const uint32_t dst = s_dst[d] + (p - s_start[d]);
        keys_out[dst] = k;
        if (kVals) vals_out[dst] = s_val[p];
    }
}

// ---- dedupe and levels: flags over a sorted list, counted per tile, scanned (exclusive_scan), written at the prefix -------------
// dedupe: the last entry of each run of equal keys.  level: the first entry of each run of equal key >> 3.
template <bool kLast> __device__ __forceinline__ bool flag_at(const uint64_t* k, uint32_t n, uint32_t i) {
    if (kLast) return i + 1u == n || k[i] != k[i + 1u];
    return i == 0u || (k[i] >> 3) != (k[i - 1u] >> 3);
}

template <bool kLast> __global__ __launch_bounds__(kThreads) void flag_count_kernel(const uint64_t* keys, uint32_t n, uint64_t* part) {
    __shared__ uint32_t lds[kWaves];
    const size_t base = size_t(blockIdx.x) * kTile;
    uint32_t sum = 0;
#pragma unroll 4
    for (uint32_t j = 0; j < kItems; j++) {
        const size_t i = base + j * kThreads + threadIdx.x;
        if (i < n) sum += flag_at<kLast>(keys, n, uint32_t(i)) ? 1u : 0u;
    }
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < kWaves; w++) all += lds[w];
        part[blockIdx.x] = all;
    }
}

__global__ __launch_bounds__(kThreads) void dedupe_write_kernel(const uint64_t* keys, const uint32_t* vals, uint32_t n, const uint64_t* part,
                                                                uint64_t* ukeys, int32_t* leaves) {
    __shared__ uint32_t lds[kWaves];
    const size_t base = size_t(blockIdx.x) * kTile;
    uint64_t at = part[blockIdx.x];
#pragma unroll 1
    for (uint32_t j = 0; j < kItems; j++) {
        const size_t i = base + j * kThreads + threadIdx.x;
        const bool keep = i < n && flag_at<true>(keys, n, uint32_t(i));
        uint32_t total;
        const uint64_t o = at + block_exclusive<uint32_t, kWaves>(keep ? 1u : 0u, lds, &total);
        at += total;
        if (keep) {
            ukeys[o] = keys[i];
            if (vals) leaves[o] = int32_t(vals[i]);   // uniform: a clear list has no values
        }
    }
}

// bins[bin * blocks + block]: entries of the block that open nodes at levels 1 .. bin (the first entry: all top + 1 levels)
__global__ __launch_bounds__(kThreads) void level_hist_kernel(const uint64_t* keys, uint32_t n, uint32_t top, uint32_t blocks, uint64_t* bins) {
    __shared__ uint32_t lds[kLevelBins][kWaves];
    const size_t base = size_t(blockIdx.x) * kTile;
    uint32_t cnt[kLevelBins];
#pragma unroll
    for (uint32_t b = 0; b < kLevelBins; b++) cnt[b] = 0u;
#pragma unroll 4
    for (uint32_t j = 0; j < kItems; j++) {
        const size_t i = base + j * kThreads + threadIdx.x;
        if (i >= n) continue;
        uint32_t lv = top;
        if (i != 0) {
            const uint64_t x = keys[i] ^ keys[i - 1];                   // != 0: the keys are unique
            lv = (63u - uint32_t(__clzll(int64_t(x)))) / 3u;            // x >> 3j != 0  <=>  j <= (highest bit) / 3
        }
#pragma unroll
        for (uint32_t b = 0; b < kLevelBins; b++) cnt[b] += lv == b ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t b = 0; b < kLevelBins; b++) {
        const uint32_t s = wave_sum(cnt[b]);
        if ((threadIdx.x & 63u) == 0u) lds[b][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < kLevelBins) {
        uint32_t all = 0;
        for (uint32_t w = 0; w < kWaves; w++) all += lds[threadIdx.x][w];
        bins[size_t(threadIdx.x) * blocks + blockIdx.x] = all;
    }
}

// one workgroup per bin: out[bin] = the sum of its row
__global__ __launch_bounds__(kRowThreads) void level_sum_kernel(const uint64_t* bins, uint32_t blocks, uint64_t* out) {
    __shared__ uint64_t lds[kRowThreads / 64];
    const uint64_t* row = bins + size_t(blockIdx.x) * blocks;
    uint64_t sum = 0;
    for (uint32_t k = threadIdx.x; k < blocks; k += kRowThreads) sum += row[k];
    sum = wave_sum(sum);
    if ((threadIdx.x & 63u) == 0u) lds[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t all = 0;
        for (uint32_t w = 0; w < kRowThreads / 64; w++) all += lds[w];
        out[blockIdx.x] = all;
    }
}

// The nodes one level up from `keys` (the level below, n entries, ascending): one per run of key >> 3, at rec_start + its rank.
// leaf: the level below is the leaf words, so base = the run's first index; otherwise base = child_start + that index.
__global__ __launch_bounds__(kThreads) void level_write_kernel(const uint64_t* keys, uint32_t n, const uint64_t* part, uint64_t* next,
                                                               SvoRecord* recs, uint64_t rec_start, uint64_t child_start, uint32_t leaf) {
    __shared__ uint32_t lds[kWaves];
    const size_t base = size_t(blockIdx.x) * kTile;
    uint64_t at = part[blockIdx.x];
#pragma unroll 1
    for (uint32_t j = 0; j < kItems; j++) {
        const size_t i = base + j * kThreads + threadIdx.x;
        const bool head = i < n && flag_at<false>(keys, n, uint32_t(i));
        uint32_t total;
        const uint64_t o = at + block_exclusive<uint32_t, kWaves>(head ? 1u : 0u, lds, &total);
        at += total;
        if (!head) continue;
        const uint64_t parent = keys[i] >> 3;
        uint32_t mask = 0;
        for (size_t c = i; c < n && c < i + 8 && (keys[c] >> 3) == parent; c++) mask |= 1u << uint32_t(keys[c] & 7u);
        SvoRecord r;
        r.masks = leaf ? mask << 8 : mask;
        r.base = uint32_t(leaf ? i : child_start + i);
        recs[rec_start + o] = r;
        if (next) next[o] = parent;
    }
}

// one workgroup: part[0 .. blocks) -> exclusive prefix sums in place, part[blocks] = the total.  Each pass takes 8 consecutive
// partials per thread.
__global__ __launch_bounds__(kScanThreads) void exclusive_scan_kernel(uint64_t* part, uint32_t blocks) {
    __shared__ uint64_t lds[kScanThreads / 64];
    uint64_t carry = 0;
    for (uint32_t c = 0; c < blocks; c += kScanThreads * kScanItems) {
        const uint32_t i0 = c + threadIdx.x * kScanItems;
        uint64_t v[kScanItems], mine = 0;
#pragma unroll
        for (uint32_t k = 0; k < kScanItems; k++) {
            v[k] = i0 + k < blocks ? part[i0 + k] : 0ull;
            mine += v[k];
        }
        uint64_t total;
        uint64_t run = carry + block_exclusive<uint64_t, kScanThreads / 64>(mine, lds, &total);
#pragma unroll
        for (uint32_t k = 0; k < kScanItems; k++) {
            if (i0 + k < blocks) part[i0 + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) part[blocks] = carry;
}

}  // namespace

hipError_t launch_exclusive_scan(uint64_t* part, uint32_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, part, blocks);
    return hipGetLastError();
}

size_t radix_hist_entries(size_t n) { return size_t(kDigits) * tiles(n); }

hipError_t radix_sort_pairs(uint64_t* keys[2], uint32_t* vals[2], uint32_t n, uint32_t bits, uint32_t* hist, uint32_t* totals, hipStream_t s,
                            int* cur) {
    const uint32_t blocks = tiles(n);
    for (uint32_t shift = 0; shift < bits; shift += 8u) {
        const int c = *cur;
        hipLaunchKernelGGL(radix_hist_kernel, dim3(blocks), dim3(kThreads), 0, s, keys[c], n, shift, blocks, hist);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL(radix_scan_kernel, dim3(kDigits), dim3(kRowThreads), 0, s, hist, blocks, totals);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        if (vals[0] != nullptr)
            hipLaunchKernelGGL(radix_scatter_kernel<true>, dim3(blocks), dim3(kThreads), 0, s, keys[c], vals[c], keys[c ^ 1], vals[c ^ 1], n,
                               shift, blocks, hist, totals);
        else
            hipLaunchKernelGGL(radix_scatter_kernel<false>, dim3(blocks), dim3(kThreads), 0, s, keys[c], nullptr, keys[c ^ 1], nullptr, n,
                               shift, blocks, hist, totals);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        *cur = c ^ 1;
    }
    return hipSuccess;
}

size_t level_part_entries(size_t m) { return size_t(tiles(m)) + 1; }
size_t level_bin_entries(size_t m) { return size_t(kLevelBins) * tiles(m) + kLevelBins; }

int build_levels(uint64_t* ukeys, uint64_t* spare, size_t m, uint64_t* part, uint64_t* bins, uint32_t depth, ScratchBuffer* leaves,
                 hipStream_t s, const char* who, DeviceTree* out) {
    ScratchBuffer svo, own_spare;
    const std::string w(who);
    // every level's node count: level j (1 = the leaf parents .. depth + 1 = the root) has the unique keys that open a node there
    const uint32_t mm = uint32_t(m), ublocks = tiles(m), top = depth + 1u;
    hipLaunchKernelGGL(level_hist_kernel, dim3(ublocks), dim3(kThreads), 0, s, ukeys, mm, top, ublocks, bins);
    HIP_TRY(hipGetLastError());
    uint64_t* bin_sums = bins + size_t(kLevelBins) * ublocks;
    hipLaunchKernelGGL(level_sum_kernel, dim3(kLevelBins), dim3(kRowThreads), 0, s, bins, ublocks, bin_sums);
    HIP_TRY(hipGetLastError());
    uint64_t bin[kLevelBins];
    HIP_TRY(hipMemcpyAsync(bin, bin_sums, sizeof bin, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t level_count[kLevelBins + 1] = {};   // [j], j = 1 .. top: the keys that open a node at level j or higher
    level_count[top] = bin[top];
    for (uint32_t j = top - 1u; j >= 1u; j--) level_count[j] = level_count[j + 1] + bin[j];
    uint64_t level_start[kLevelBins + 2] = {};   // top-down: the root's level first
    uint64_t nodes = 0;
    for (uint32_t j = top; j >= 1u; j--) { level_start[j] = nodes; nodes += level_count[j]; }
    if (level_count[top] != 1u) { set_error(w + ": internal error: the root level has " + std::to_string(level_count[top]) + " nodes"); return VXRT_E_SCENE; }
    if (nodes > 0xffffffffull) { set_error(w + ": " + std::to_string(nodes) + " octree nodes: 2^32 or more"); return VXRT_E_SCENE; }
    if (spare == nullptr && top > 1u) {   // the levels above the leaf parents ping-pong between ukeys and a buffer of the leaf parents' size
        if (int rc = alloc_scratch(&own_spare, size_t(level_count[1]) * sizeof(uint64_t), who, "the node keys")) return rc;
        spare = own_spare.as<uint64_t>();
    }
    if (int rc = alloc_scratch(&svo, size_t(nodes) * sizeof(SvoRecord), who, "the records")) return rc;

    // the levels, bottom-up, each written at its top-down place
    uint64_t* buf[2] = {ukeys, spare};
    int cur = 0;
    uint32_t below = mm;   // entries of the level below (the unique keys, then level j's nodes)
    for (uint32_t j = 1; j <= top; j++) {
        const uint32_t lb = tiles(below);
        const uint64_t* in = buf[cur];
        uint64_t* next = j < top ? buf[cur ^ 1] : nullptr;
        hipLaunchKernelGGL(flag_count_kernel<false>, dim3(lb), dim3(kThreads), 0, s, in, below, part);
        HIP_TRY(hipGetLastError());
        HIP_TRY(launch_exclusive_scan(part, lb, s));
        hipLaunchKernelGGL(level_write_kernel, dim3(lb), dim3(kThreads), 0, s, in, below, part, next, svo.as<SvoRecord>(),
                           level_start[j], j == 1u ? 0ull : level_start[j - 1], j == 1u ? 1u : 0u);
        HIP_TRY(hipGetLastError());
        below = uint32_t(level_count[j]);
        cur ^= 1;
    }
    SvoRecord root;
    HIP_TRY(hipMemcpyAsync(&root, svo.get(), sizeof root, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));

    out->svo = static_cast<SvoRecord*>(svo.release()); out->svo_count = size_t(nodes);
    out->leaves = static_cast<int32_t*>(leaves->release()); out->leaf_count = m;
    out->depth = depth;
    out->root = root;
    return VXRT_OK;
}

int build_empty_tree(hipStream_t s, const char* who, DeviceTree* out) {
    *out = DeviceTree{};
    // the host builder's empty tree: the root {masks 0, base 1} and one zero leaf word (api_scene.hip: upload_svo)
    ScratchBuffer svo, leaves;
    const SvoRecord root{0u, 1u};
    const int32_t zero = 0;
    if (int rc = alloc_scratch(&svo, sizeof root, who, "the records")) return rc;
    if (int rc = alloc_scratch(&leaves, sizeof zero, who, "the leaf words")) return rc;
    HIP_TRY(hipMemcpyAsync(svo.get(), &root, sizeof root, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(leaves.get(), &zero, sizeof zero, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    out->svo = static_cast<SvoRecord*>(svo.release()); out->svo_count = 1;
    out->leaves = static_cast<int32_t*>(leaves.release()); out->leaf_count = 1;
    out->root = root;
    return VXRT_OK;
}

int KeySort::alloc(size_t n, bool with_vals, const char* who, const char* keys_name, const char* vals_name) {
    for (int b = 0; b < 2; b++) {
        if (int rc = alloc_scratch(&key[b], n * sizeof(uint64_t), who, keys_name)) return rc;
        if (with_vals)
            if (int rc = alloc_scratch(&val[b], n * sizeof(uint32_t), who, vals_name)) return rc;
    }
    return alloc_counts(n, who);
}

int KeySort::alloc_keys(size_t entries, const char* who, const char* name) {
    for (int b = 0; b < 2; b++)
        if (int rc = alloc_scratch(&key[b], entries * sizeof(uint64_t), who, name)) return rc;
    return VXRT_OK;
}

int KeySort::alloc_counts(size_t n, const char* who) {
    if (int rc = alloc_scratch(&hist, radix_hist_entries(n) * sizeof(uint32_t), who, "the digit counts")) return rc;
    return alloc_scratch(&totals, kDigits * sizeof(uint32_t), who, "the digit counts");
}

hipError_t KeySort::sort(uint32_t n, uint32_t bits, hipStream_t s) {
    uint64_t* kp[2] = {key[0].as<uint64_t>(), key[1].as<uint64_t>()};
    uint32_t* vp[2] = {val[0].as<uint32_t>(), val[1].as<uint32_t>()};
    return radix_sort_pairs(kp, vp, n, bits, hist.as<uint32_t>(), totals.as<uint32_t>(), s, &at);
}

int alloc_list_scratch(size_t n, bool with_vals, const char* who, ListScratch* ls) {
    if (int rc = ls->alloc(n, with_vals, who)) return rc;
    return alloc_scratch(&ls->part, (size_t(tiles(n)) + 1) * sizeof(uint64_t), who, "the scan partials");
}

int sort_unique_list(ListScratch* ls, uint32_t n, uint32_t depth, ScratchBuffer* leaves, hipStream_t s, const char* who, size_t* m_out) {
    const uint32_t blocks = tiles(n);
    const bool with_vals = ls->vals() != nullptr;
    // stable LSD radix sort over the key's 3(depth + 1) bits
    HIP_TRY(ls->sort(n, 3u * (depth + 1u), s));

    // dedupe: the last entry of each key -> the leaf words (exactly sized) and the unique keys (the spare side)
    uint64_t* part = ls->part.as<uint64_t>();
    hipLaunchKernelGGL(flag_count_kernel<true>, dim3(blocks), dim3(kThreads), 0, s, ls->keys(), n, part);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_exclusive_scan(part, blocks, s));
    uint64_t m = 0;
    HIP_TRY(hipMemcpyAsync(&m, part + blocks, sizeof m, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (with_vals)
        if (int rc = alloc_scratch(leaves, size_t(m) * sizeof(int32_t), who, "the leaf words")) return rc;
    hipLaunchKernelGGL(dedupe_write_kernel, dim3(blocks), dim3(kThreads), 0, s, ls->keys(), ls->vals(), n, part, ls->spare_keys(),
                       with_vals ? leaves->as<int32_t>() : nullptr);
    HIP_TRY(hipGetLastError());
    ls->flip();
    *m_out = size_t(m);
    return VXRT_OK;
}

int build_svo_device_list(const int16_t* pos, const uint8_t* mrgb, size_t n, hipStream_t s, DeviceTree* out) {
    *out = DeviceTree{};
    const char* who = "vxrt_set_voxels_device";
    ScratchBuffer leaves;
    if (n == 0) return build_empty_tree(s, who, out);
    const uint32_t nn = uint32_t(n);   // the caller refuses n >= 2^32

    // bounds -> depth
    ScratchBuffer bpart;
    if (int rc = alloc_scratch(&bpart, (kBoundsBlocks + 1) * sizeof(int2), who, "the scratch")) return rc;
    const uint32_t vec = (reinterpret_cast<uintptr_t>(pos) & 15u) == 0u ? 1u : 0u;
    hipLaunchKernelGGL(bounds_kernel, dim3(kBoundsBlocks), dim3(kThreads), 0, s, pos, 3 * n, vec, bpart.as<int2>());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(bounds_reduce_kernel, dim3(1), dim3(kThreads), 0, s, bpart.as<int2>(), kBoundsBlocks);
    HIP_TRY(hipGetLastError());
    int2 lohi;
    HIP_TRY(hipMemcpyAsync(&lohi, bpart.as<int2>() + kBoundsBlocks, sizeof lohi, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t depth = depth_of_bounds(lohi.x, lohi.y);
    if (depth > 15) { set_error("octree depth > 15"); return VXRT_E_SCENE; }

    // scratch: keys and leaf words double-buffered, the digit counts, the scan partials, the level bins
    const uint32_t blocks = tiles(n);
    ListScratch ls;
    ScratchBuffer bins;
    if (int rc = alloc_list_scratch(n, true, who, &ls)) return rc;
    if (int rc = alloc_scratch(&bins, (size_t(kLevelBins) * blocks + kLevelBins) * sizeof(uint64_t), who, "the level counts")) return rc;

    const uint32_t words = (reinterpret_cast<uintptr_t>(mrgb) & 3u) == 0u ? 1u : 0u;
    hipLaunchKernelGGL(keys_kernel, dim3(uint32_t((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, pos, mrgb, n, depth, words,
                       ls.keys(), ls.vals());
    HIP_TRY(hipGetLastError());

    size_t m = 0;
    if (int rc = sort_unique_list(&ls, nn, depth, &leaves, s, who, &m)) return rc;
    return build_levels(ls.keys(), ls.spare_keys(), m, ls.part.as<uint64_t>(), bins.as<uint64_t>(), depth,
                        &leaves, s, who, out);
}


}  // namespace vxrt
