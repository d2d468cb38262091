// api_components.hip — host side of vxrt_components.h: the connected components of a voxel list in device memory, and the voxels of
// the loaded scene that hang on nothing inside an anchor box.  The labelling is here: the sort and the scans are the list builder's
// (device_build.h), everything between is components.hip.  The two entry points are vxrt_pieces.h's with less asked of them, so each
// shares its body with its twin (pieces.h: component_table, detached_pieces).  DESIGN.md §20.
#include "pieces.h"
#include "../../include/vxrt_components.h"

namespace vxrt {

// About 40 bytes per entry, all of it allocated before the first launch.
int alloc_labelling(size_t n, const char* who, Labelling* l) {
    if (int rc = l->ls.alloc(n, true, who)) return rc;
    for (ScratchBuffer* b : {&l->uhead, &l->parent, &l->comp, &l->acc})
        if (int rc = alloc_scratch(b, n * sizeof(uint32_t), who, "the union-find")) return rc;
    return alloc_scratch(&l->part, (size_t(comp_blocks(n)) + 1) * sizeof(uint64_t), who, "the scan partials");
}

// pos[0 .. n), 0 < n < 2^32, read on s -> *l.  axes: 1, 2 or 3.  Waits for the two counts.
int label_list(const int16_t* pos, uint32_t n, uint32_t axes, const CompBox& box, hipStream_t s, Labelling* l) {
    KeySort& ls = l->ls;
    uint64_t* part = l->part.as<uint64_t>();
    HIP_TRY(components_keys(pos, n, ls.keys(), ls.vals(), s));
    HIP_TRY(ls.sort(n, kCompKeyBits, s));
    // the sort's other buffers are free from here on: they take the unique keys and the entries' ranks
    uint64_t* ukeys = ls.spare_keys();
    uint32_t* rank = ls.spare_vals();
    HIP_TRY(components_heads_count(ls.keys(), n, part, s));
    HIP_TRY(launch_exclusive_scan(part, comp_blocks(n), s));
    uint64_t m = 0;
    HIP_TRY(hipMemcpyAsync(&m, part + comp_blocks(n), sizeof m, hipMemcpyDeviceToHost, s));
    HIP_TRY(components_heads_write(ls.keys(), ls.vals(), n, part, ukeys, l->uhead.as<uint32_t>(), rank, l->parent.as<uint32_t>(), l->acc.as<uint32_t>(), s));
    HIP_TRY(hipStreamSynchronize(s));      // m; the partials are rewritten below
    const uint32_t mm = uint32_t(m);       // 0 < m <= n
    HIP_TRY(components_union(ukeys, mm, axes, l->parent.as<uint32_t>(), s));
    HIP_TRY(components_flatten(ukeys, l->uhead.as<uint32_t>(), l->parent.as<uint32_t>(), mm, box, l->comp.as<uint32_t>(), l->acc.as<uint32_t>(), part, s));
    HIP_TRY(launch_exclusive_scan(part, comp_blocks(mm), s));
    HIP_TRY(hipMemcpyAsync(&l->components, part + comp_blocks(mm), sizeof l->components, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    l->ukeys = ukeys;
    l->sorted = ls.vals();
    l->rank = rank;
    l->unique = mm;
    return VXRT_OK;
}

// 6, 18, 26 -> the axes on which two neighbours may differ; anything else -> 0
uint32_t axes_of(uint32_t connectivity) { return connectivity == 6u ? 1u : connectivity == 18u ? 2u : connectivity == 26u ? 3u : 0u; }

}  // namespace vxrt

extern "C" {

int vxrt_label_components_device(vxrt_ctx* c, const int16_t (*pos)[3], size_t n, uint32_t connectivity, uint32_t* label,
                                 size_t* n_components) try {
    return vxrt::component_table("vxrt_label_components_device", c, pos, n, connectivity, label, nullptr, nullptr, 0, n_components);
} VXRT_CATCH

int vxrt_detached_voxels_device(vxrt_ctx* c, const int32_t anchor_min[3], const int32_t anchor_max[3], uint32_t connectivity,
                                int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap, size_t* n) try {
    return vxrt::detached_pieces("vxrt_detached_voxels_device", c, anchor_min, anchor_max, connectivity, 0u, 0xffffffffu, pos, mrgb, nullptr, cap,
                                 n, nullptr, 0, nullptr);
} VXRT_CATCH

}  // extern "C"
