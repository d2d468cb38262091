// api_voxelize.hip — host side of vxrt_voxelize.h: a triangle mesh in device memory -> a voxel list in device memory.  The front is
// voxelize.hip (setup, the counting walk, the emitting walk), the middle is the list builder's sort and keep-last dedupe
// (device_build.hip: sort_unique_list; it is stable, so the highest triangle index wins a shared voxel), the end is voxelize.hip's
// decode into the caller's arrays.  Nothing but the summary and three counts crosses to the host.  DESIGN.md §17.
// The argument checks, the setup pass with its refusals, the key depth and the way out into the caller's arrays are functions of
// their own (voxelize.h), because vxrt_voxelize_solid_device (api_solid.hip) takes the same mesh and gives the same kind of list.
#include <string>

#include "ctx.h"
#include "device_build.h"
#include "scene_args.h"
#include "voxelize.h"
#include "../../include/vxrt_voxelize.h"

namespace vxrt {

int voxelize_check_args(vxrt_ctx* c, const char* who, const void* verts, size_t n_verts, const void* tris, const void* tri_mrgb, size_t n_tris,
                        const void* pos, const void* mrgb, size_t cap) {
    if (!tris) { set_error(std::string(who) + ": null triangles"); return VXRT_E_INVALID; }
    if (n_verts != 0 && !verts) { set_error(std::string(who) + ": null vertices"); return VXRT_E_INVALID; }
    if ((reinterpret_cast<uintptr_t>(verts) & 3u) != 0u || (reinterpret_cast<uintptr_t>(tris) & 3u) != 0u) {
        set_error(std::string(who) + ": verts and tris must be 4-byte aligned");
        return VXRT_E_INVALID;
    }
    if (n_verts > SIZE_MAX / (3 * sizeof(float))) { set_error(std::string(who) + ": too many vertices"); return VXRT_E_INVALID; }
    HIP_TRY(hipSetDevice(c->cfg.device));
    if (n_verts != 0)
        if (int rc = check_device_array(c, verts, n_verts * 3 * sizeof(float), who, "verts")) return rc;
    if (int rc = check_device_array(c, tris, n_tris * 3 * sizeof(uint32_t), who, "tris")) return rc;
    if (tri_mrgb)
        if (int rc = check_device_array(c, tri_mrgb, n_tris * 4, who, "tri_mrgb")) return rc;
    if (pos != nullptr && cap != 0) {
        if (int rc = check_device_array(c, pos, cap * 3 * sizeof(int16_t), who, "pos")) return rc;
        if (int rc = check_device_array(c, mrgb, cap * 4, who, "mrgb")) return rc;
    }
    return VXRT_OK;
}

int voxelize_front(const char* who, const void* verts, size_t n_verts, const void* tris, size_t n_tris, hipStream_t s, MeshFront* f) {
    const uint32_t tblocks = vox_blocks(n_tris);
    if (int rc = alloc_scratch(&f->tq, n_tris * sizeof(VoxTri), who, "the snapped triangles")) return rc;
    if (int rc = alloc_scratch(&f->off, (n_tris + 1) * sizeof(uint64_t), who, "the column offsets")) return rc;
    if (int rc = alloc_scratch(&f->tpart, (size_t(tblocks) + 1) * sizeof(uint64_t), who, "the scan partials")) return rc;
    if (int rc = alloc_scratch(&f->bounds, (size_t(tblocks) + 1) * sizeof(MeshSummary), who, "the bounds")) return rc;
    if (int rc = voxelize_setup(static_cast<const float*>(verts), n_verts, static_cast<const uint32_t*>(tris), n_tris, f->tq.as<VoxTri>(),
                                f->off.as<uint64_t>(), f->tpart.as<uint64_t>(), f->bounds.as<MeshSummary>(), s, &f->ms, &f->columns))
        return rc;
    const MeshSummary& ms = f->ms;
    if (ms.flags & kVoxBadIndex) {
        set_error(std::string(who) + ": a triangle names a vertex index >= n_verts (" + std::to_string(n_verts) + ")");
        return VXRT_E_INVALID;
    }
    if (ms.flags & kVoxNotFinite) { set_error(std::string(who) + ": a vertex used by a triangle is not finite"); return VXRT_E_INVALID; }
    if (ms.flags & kVoxOutside) {
        set_error(std::string(who) + ": the mesh spans voxels [" + std::to_string(ms.lo[0]) + ", " + std::to_string(ms.hi[0]) + "] x [" +
                  std::to_string(ms.lo[1]) + ", " + std::to_string(ms.hi[1]) + "] x [" + std::to_string(ms.lo[2]) + ", " + std::to_string(ms.hi[2]) +
                  "] (clamped to +-2^26): a vertex snaps outside [" + std::to_string(kVoxSnapLo) + ", " + std::to_string(kVoxSnapHi) +
                  ") sixteenths of a voxel, [-32768, 32768) voxels");
        return VXRT_E_SCENE;
    }
    return VXRT_OK;
}

uint32_t voxelize_depth(const MeshSummary& ms) {
    uint32_t depth = 0;      // the least whose cube [-2^depth, 2^depth)^3 holds the candidate cells: at most 15
    for (int ax = 0; ax < 3; ax++)
        while (ms.lo[ax] < -(int32_t(1) << depth) || ms.hi[ax] >= (int32_t(1) << depth)) depth++;
    return depth;
}

int voxelize_output(const char* who, const uint64_t* keys, const int32_t* words, size_t m, uint32_t depth, void* pos, void* mrgb, size_t cap,
                    hipStream_t s, size_t* n) {
    if (pos == nullptr) {
        HIP_TRY(hipStreamSynchronize(s));      // the dedupe's write into the scratch, before the scratch is freed
        *n = m;
        return VXRT_OK;
    }
    if (cap < m) {
        HIP_TRY(hipStreamSynchronize(s));
        *n = m;
        set_error(std::string(who) + ": " + std::to_string(m) + " voxels, room for " + std::to_string(cap));
        return VXRT_E_INVALID;
    }
    ScratchBuffer stage[2];
    if (int rc = write_voxels_staged(pos, mrgb, m, s, who, stage, [&](int16_t* dst_pos, uint32_t* dst_mrgb) {
            return voxelize_decode(keys, words, uint32_t(m), depth, dst_pos, dst_mrgb, s);
        }))
        return rc;
    HIP_TRY(hipStreamSynchronize(s));
    *n = m;
    return VXRT_OK;
}

}  // namespace vxrt

extern "C" {

int vxrt_voxelize_mesh_device(vxrt_ctx* c, const float (*verts)[3], size_t n_verts, const uint32_t (*tris)[3], const uint8_t (*tri_mrgb)[4],
                              size_t n_tris, int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap, size_t* n) try {
    using namespace vxrt;
    const char* who = "vxrt_voxelize_mesh_device";
    if (!valid_ctx(c) || !n) { set_error("null argument"); return VXRT_E_INVALID; }
    if ((pos == nullptr) != (mrgb == nullptr)) { set_error("pos and mrgb: both or neither"); return VXRT_E_INVALID; }
    const bool count_only = pos == nullptr;
    if (uint64_t(n_tris) >= (uint64_t(1) << 32)) { set_error(std::string(who) + ": 2^32 triangles or more"); return VXRT_E_INVALID; }
    if (n_tris == 0) { *n = 0; return VXRT_OK; }
    if (!count_only && !tri_mrgb) { set_error(std::string(who) + ": null tri_mrgb with output arrays"); return VXRT_E_INVALID; }
    if (int rc = voxelize_check_args(c, who, verts, n_verts, tris, tri_mrgb, n_tris, pos, mrgb, cap)) return rc;

    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    const uint32_t nt = uint32_t(n_tris);
    MeshFront f;
    if (int rc = voxelize_front(who, verts, n_verts, tris, n_tris, s, &f)) return rc;
    const uint64_t limit = uint64_t(1) << 32, columns = f.columns;
    if (columns >= limit) {
        set_error(std::string(who) + ": " + std::to_string(columns) + " candidate columns (the limit is 2^32, for them and for the overlaps, which were not counted)");
        return VXRT_E_SCENE;
    }
    const uint32_t cblocks = vox_blocks(columns);
    ScratchBuffer cpart;
    if (int rc = alloc_scratch(&cpart, (size_t(cblocks) + 1) * sizeof(uint64_t), who, "the scan partials")) return rc;
    uint64_t hits = 0;
    if (int rc = voxelize_count(f.tq.as<VoxTri>(), f.off.as<uint64_t>(), nt, uint32_t(columns), cpart.as<uint64_t>(), s, &hits)) return rc;
    if (hits >= limit) {
        set_error(std::string(who) + ": " + std::to_string(hits) + " triangle-cell overlaps in " + std::to_string(columns) +
                  " candidate columns (the limit is 2^32 for each)");
        return VXRT_E_SCENE;
    }
    if (hits == 0) { *n = 0; return VXRT_OK; }      // cannot happen (a triangle meets the cell of its first vertex); kept for the kernels' sake

    // the keys at the depth of the candidate cells' bounds: the order is the same at every depth that holds the list
    const uint32_t depth = voxelize_depth(f.ms);
    ListScratch ls;
    if (int rc = alloc_list_scratch(size_t(hits), !count_only, who, &ls)) return rc;
    HIP_TRY(voxelize_emit(f.tq.as<VoxTri>(), f.off.as<uint64_t>(), nt, uint32_t(columns), cpart.as<uint64_t>(), depth,
                          reinterpret_cast<const uint8_t*>(tri_mrgb), ls.keys(), ls.vals(), s));
    ScratchBuffer words;
    size_t m = 0;
    if (int rc = sort_unique_list(&ls, uint32_t(hits), depth, &words, s, who, &m)) return rc;
    return voxelize_output(who, ls.keys(), words.as<int32_t>(), m, depth, pos, mrgb, cap, s, n);
} VXRT_CATCH

}  // extern "C"
