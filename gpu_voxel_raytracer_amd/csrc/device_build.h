// device_build.h — what api_device_scene.hip (host side of vxrt_device_scene.h), device_build.hip (the list builder), grid_build.hip
// (the dense-grid builder), grid_edit.hip (the grid editor), api_grid.hip (host side of vxrt_grid.h) and api_device_edit.hip /
// device_edit.hip (vxrt_device_edit.h) share, and the device primitives they and api_extract.hip use: the path key and leaf word,
// lanes_below, the exclusive scan, the radix sort, the holder of its two sides that every sorting site uses (KeySort) and the
// sort-and-dedupe front of a list (device_build.hip).  The front at depth 15 behind the list operators, the scan with its total
// read back and the run heads of sorted keys are list_ops.h's key_list, scan_total and run_heads over these; api_device_edit.hip,
// api_voxelize.hip and api_solid.hip run the front at a depth of their own.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "ctx.h"
#include "kernels.h"

namespace vxrt {

// A scene built on the device from a voxel list: the 8-byte records and leaf words that flatten_svo(build_octree(list)) gives,
// byte for byte.  The arrays are the caller's (hipMalloc'd, exactly sized) once the build returned VXRT_OK.
struct DeviceTree {
    SvoRecord* svo = nullptr;
    size_t svo_count = 0;
    int32_t* leaves = nullptr;
    size_t leaf_count = 0;
    uint32_t depth = 0;
    SvoRecord root{0, 0};
};

// pos / mrgb: n entries in device memory of the current device, read on `stream` behind what is enqueued there.  Waits for the
// result.  VXRT_E_SCENE: depth > 15 or 2^32 records or more; VXRT_E_DEVICE: an allocation or launch failed.  Nothing is allocated
// on failure.  The pipeline is in device_build.hip and DESIGN.md §11.
int build_svo_device_list(const int16_t* pos, const uint8_t* mrgb, size_t n, hipStream_t stream, DeviceTree* out);

// The host builder's empty tree (the root {masks 0, base 1} and one zero leaf word).  `who` names the API call in error messages.
int build_empty_tree(hipStream_t stream, const char* who, DeviceTree* out);

// The lanes of this wave below this one whose bit is set in m (a ballot): this lane's rank among them.
__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi(uint32_t(m >> 32), __builtin_amdgcn_mbcnt_lo(uint32_t(m), 0u));
}

// A voxel's path key at depth d, u = p + 2^d per axis: bit k of u lands at bits 3k + 2 (x), 3k + 1 (y), 3k (z), k = 0 .. d — the key
// vxrt_edit_voxels sorts by (api_edit.hip: path_key) and the order of the records (vxrt_extract.h).
__device__ __forceinline__ uint64_t path_key_of(uint32_t ux, uint32_t uy, uint32_t uz, uint32_t depth) {
    uint64_t key = 0;
    for (uint32_t k = 0; k <= depth; k++)
        key |= uint64_t(((ux >> k) & 1u) << 2 | ((uy >> k) & 1u) << 1 | ((uz >> k) & 1u)) << (3u * k);
    return key;
}

// scene_host.cpp: build_octree's leaf word of (material, r, g, b)
__device__ __forceinline__ uint32_t leaf_word_of(uint32_t m, uint32_t r, uint32_t g, uint32_t b) {
    return 0x80000000u | (m & 0x7fu) << 24 | r << 16 | g << 8 | b;
}

// One workgroup: part[0 .. blocks) -> its exclusive prefix sums in place, part[blocks] = the total.
hipError_t launch_exclusive_scan(uint64_t* part, uint32_t blocks, hipStream_t stream);

// Stable LSD radix sort of (keys, vals), n entries, over the low `bits` key bits, 8 per pass, ping-ponging between keys[0] / vals[0]
// and keys[1] / vals[1] starting at [*cur]; the result is in [*cur] on return.  vals[0] == nullptr: keys only.  hist: radix_hist_entries(n) words; totals: 256 words.
size_t radix_hist_entries(size_t n);
hipError_t radix_sort_pairs(uint64_t* keys[2], uint32_t* vals[2], uint32_t n, uint32_t bits, uint32_t* hist, uint32_t* totals,
                            hipStream_t stream, int* cur);

// The buffers of one such sort and which side is which: keys() / vals() are the side the next launch writes before the sort and
// the sorted side after it, spare_keys() / spare_vals() the other, free for the caller once the sort is enqueued.  vals() is null
// without values, and the sort then moves keys only.
struct KeySort {
    ScratchBuffer key[2], val[2], hist, totals;
    int at = 0;
    // n entries a side (keys, and with_vals values) and the digit counts.  The names are what a failed allocation says.
    int alloc(size_t n, bool with_vals, const char* who, const char* keys_name = "the keys", const char* vals_name = "the leaf words");
    // The pieces, for a caller that wants other sizes: `entries` keys a side and no values; the digit counts of a sort of n entries.
    int alloc_keys(size_t entries, const char* who, const char* name);
    int alloc_counts(size_t n, const char* who);
    uint64_t* keys() const { return key[at].as<uint64_t>(); }
    uint32_t* vals() const { return val[at].as<uint32_t>(); }
    uint64_t* spare_keys() const { return key[at ^ 1].as<uint64_t>(); }
    uint32_t* spare_vals() const { return val[at ^ 1].as<uint32_t>(); }
    // The spare side becomes keys() / vals(): for a caller that wrote its result there (sort_unique_list's dedupe, distance's tiles).
    void flip() { at ^= 1; }
    // radix_sort_pairs over the low `bits` bits of keys()[0 .. n); keys() / vals() are the result from then on.  Does not wait.
    hipError_t sort(uint32_t n, uint32_t bits, hipStream_t stream);
};

// The front half the list builder and vxrt_edit_voxels_device share, behind their own key pass: the scratch of a list of n entries
// (a KeySort and the scan partials: about 24 bytes per entry), then the stable sort of keys() / vals() over the 3(depth + 1) key
// bits and the keep-last dedupe into the spare side, which becomes keys().  On return the m unique keys are ascending in keys(),
// spare_keys() is free, and with values *leaves holds their m leaf words (exactly sized); a list without values (vals
// not allocated) leaves *leaves alone.  Waits for the count.  VXRT_E_DEVICE: an allocation failed.
struct ListScratch : KeySort {
    ScratchBuffer part;
};
int alloc_list_scratch(size_t n, bool with_vals, const char* who, ListScratch* ls);
int sort_unique_list(ListScratch* ls, uint32_t n, uint32_t depth, ScratchBuffer* leaves, hipStream_t stream, const char* who, size_t* m);

// The back half of both builders: the node levels over m > 0 unique path keys in ascending order (ukeys, m < 2^32) and their leaf
// words (*leaves, exactly m int32, handed to *out on success) -> the records, one exact allocation.  ukeys is overwritten; spare
// (the level ping-pong) holds at least m keys, or is null and then allocated at the leaf parents' count.  part: level_part_entries(m),
// bins: level_bin_entries(m).  Waits for the result.  VXRT_E_SCENE: 2^32 records or more; VXRT_E_DEVICE: an allocation failed.
size_t level_part_entries(size_t m);
size_t level_bin_entries(size_t m);
int build_levels(uint64_t* ukeys, uint64_t* spare, size_t m, uint64_t* part, uint64_t* bins, uint32_t depth, ScratchBuffer* leaves,
                 hipStream_t stream, const char* who, DeviceTree* out);

// u16::next_power_of_two().trailing_zeros() of |lo| and |hi| + 1 (scene_host.cpp: build_octree's depth rule over the coordinates' min
// and max); may exceed 15
inline uint32_t depth_of_bounds(int lo, int hi) {
    auto ceil_log2_u16 = [](uint32_t v) { uint32_t bits = 0; while ((1u << bits) < v) bits++; return bits; };
    const uint32_t dlo = ceil_log2_u16(uint32_t(lo < 0 ? -lo : lo) & 0xffffu);
    const uint32_t dhi = ceil_log2_u16((uint32_t(hi < 0 ? -hi : hi) + 1u) & 0xffffu);
    return dlo > dhi ? dlo : dhi;
}

// A tree built on the device -> the context's scene: the wide records when the context asks for them, then install_scene (which
// owns the arrays from then on, or frees them on failure).  who: the API call.
int install_device_tree(vxrt_ctx* c, const DeviceTree& t, const char* who);

}  // namespace vxrt
