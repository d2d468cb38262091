// api_solid.hip — host side of vxrt_solid.h: a closed triangle mesh in device memory -> its interior, alone or under its surface, as
// a voxel list in device memory.  The mesh checks, the setup pass, the surface walk, the sort with keep-last dedupe and the decode
// are vxrt_voxelize_mesh_device's (voxelize.h, device_build.h); the crossing, pair and fill passes between them are solid.hip.
// In UNION mode the interior entries go first in the list and the surface's behind them, so the stable sort's keep-last lets the
// surface win a shared cell.  Nothing but the summary and six counts crosses to the host.  DESIGN.md §18.
#include <string>

#include "ctx.h"
#include "device_build.h"
#include "scene_args.h"
#include "solid.h"
#include "voxelize.h"
#include "../../include/vxrt_solid.h"

extern "C" {

int vxrt_voxelize_solid_device(vxrt_ctx* c, const float (*verts)[3], size_t n_verts, const uint32_t (*tris)[3], const uint8_t (*tri_mrgb)[4],
                               size_t n_tris, const uint8_t fill_mrgb[4], uint32_t mode, int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap,
                               size_t* n) try {
    using namespace vxrt;
    const char* who = "vxrt_voxelize_solid_device";
    if (!valid_ctx(c) || !n) { set_error("null argument"); return VXRT_E_INVALID; }
    if ((pos == nullptr) != (mrgb == nullptr)) { set_error("pos and mrgb: both or neither"); return VXRT_E_INVALID; }
    const bool count_only = pos == nullptr;
    if (mode != VXRT_SOLID_UNION && mode != VXRT_SOLID_INTERIOR) { set_error(std::string(who) + ": bad mode"); return VXRT_E_INVALID; }
    const bool with_surface = mode == VXRT_SOLID_UNION;
    if (!count_only && !fill_mrgb) { set_error(std::string(who) + ": null fill_mrgb with output arrays"); return VXRT_E_INVALID; }
    if (uint64_t(n_tris) >= (uint64_t(1) << 32)) { set_error(std::string(who) + ": 2^32 triangles or more"); return VXRT_E_INVALID; }
    if (n_tris == 0) { *n = 0; return VXRT_OK; }
    if (!count_only && with_surface && !tri_mrgb) {
        set_error(std::string(who) + ": null tri_mrgb with output arrays in VXRT_SOLID_UNION mode");
        return VXRT_E_INVALID;
    }
    if (int rc = voxelize_check_args(c, who, verts, n_verts, tris, tri_mrgb, n_tris, pos, mrgb, cap)) return rc;

    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    const uint32_t nt = uint32_t(n_tris);
    const uint64_t limit = uint64_t(1) << 32;
    MeshFront f;
    if (int rc = voxelize_front(who, verts, n_verts, tris, n_tris, s, &f)) return rc;
    const SolidKeying keying = solid_keying(f.ms);
    const uint32_t depth = voxelize_depth(f.ms);

    // the crossings: count, emit, sort
    ScratchBuffer zoff, zpart;
    if (int rc = alloc_scratch(&zoff, (n_tris + 1) * sizeof(uint64_t), who, "the z-column offsets")) return rc;
    if (int rc = alloc_scratch(&zpart, (size_t(vox_blocks(n_tris)) + 1) * sizeof(uint64_t), who, "the scan partials")) return rc;
    uint64_t zcolumns = 0, crossings = 0, cells = 0;
    if (int rc = solid_columns(f.tq.as<VoxTri>(), nt, zoff.as<uint64_t>(), zpart.as<uint64_t>(), s, &zcolumns)) return rc;
    if (zcolumns >= limit) {
        set_error(std::string(who) + ": " + std::to_string(zcolumns) + " z-columns over all triangles (the limit is 2^32, for them, for the crossings "
                  "and for the list's entries, which were not counted)");
        return VXRT_E_SCENE;
    }
    ScratchBuffer cpart;
    KeySort xs;      // the crossings' keys, double-buffered, and the sort's counts
    if (zcolumns != 0) {
        if (int rc = alloc_scratch(&cpart, (size_t(vox_blocks(zcolumns)) + 1) * sizeof(uint64_t), who, "the scan partials")) return rc;
        if (int rc = solid_count(f.tq.as<VoxTri>(), zoff.as<uint64_t>(), nt, uint32_t(zcolumns), cpart.as<uint64_t>(), s, &crossings)) return rc;
    }
    if (crossings >= limit) {      // cannot happen (a column gives at most one crossing); kept for the kernels' sake
        set_error(std::string(who) + ": " + std::to_string(crossings) + " crossings in " + std::to_string(zcolumns) + " z-columns (the limit is 2^32 for each)");
        return VXRT_E_SCENE;
    }
    const uint32_t pairs = uint32_t(crossings / 2);
    if (crossings != 0) {
        if (int rc = xs.alloc(size_t(crossings), false, who)) return rc;
        HIP_TRY(solid_emit(f.tq.as<VoxTri>(), zoff.as<uint64_t>(), nt, uint32_t(zcolumns), cpart.as<uint64_t>(), keying, xs.keys(), s));
        HIP_TRY(xs.sort(uint32_t(crossings), keying.bits, s));
        // the pairs: closedness and the interior lengths.  Their offsets go into the sort's other buffer, which is free from here on
        // and holds crossings >= crossings / 2 + 1 words
        ScratchBuffer ppart;
        if (int rc = alloc_scratch(&ppart, (size_t(vox_blocks(pairs)) + 1) * sizeof(uint64_t), who, "the scan partials")) return rc;
        bool closed = false;
        SolidOpen open{};
        if (int rc = solid_pairs(xs.keys(), uint32_t(crossings), keying, xs.spare_keys(), ppart.as<uint64_t>(), who, s, &closed, &open, &cells)) return rc;
        if (!closed) {
            set_error(std::string(who) + ": the mesh is not closed: column (" + std::to_string(open.x) + ", " + std::to_string(open.y) + ") is crossed " +
                      std::to_string(open.crossings) + " times, the first column in x, then y order with an odd count (" + std::to_string(crossings) +
                      " crossings in all)");
            return VXRT_E_SCENE;
        }
    }

    // the surface, counted
    uint64_t hits = 0;
    ScratchBuffer spart;
    if (with_surface) {
        if (f.columns >= limit) {
            set_error(std::string(who) + ": " + std::to_string(f.columns) + " candidate columns of the surface (the limit is 2^32)");
            return VXRT_E_SCENE;
        }
        if (int rc = alloc_scratch(&spart, (size_t(vox_blocks(f.columns)) + 1) * sizeof(uint64_t), who, "the scan partials")) return rc;
        if (int rc = voxelize_count(f.tq.as<VoxTri>(), f.off.as<uint64_t>(), nt, uint32_t(f.columns), spart.as<uint64_t>(), s, &hits)) return rc;
    }
    const uint64_t entries = cells + hits;      // cells < 2^48 and hits < 2^64 - 2^48
    if (cells >= limit || hits >= limit || entries >= limit) {
        set_error(std::string(who) + ": " + std::to_string(cells) + " interior cells and " + std::to_string(hits) +
                  " triangle-cell overlaps of the surface (the limit is 2^32 for their sum)");
        return VXRT_E_SCENE;
    }
    if (entries == 0) { *n = 0; return VXRT_OK; }      // INTERIOR mode of a mesh that encloses no cell centre

    // one list: the interior first, the surface behind it
    ListScratch ls;
    if (int rc = alloc_list_scratch(size_t(entries), !count_only, who, &ls)) return rc;
    uint64_t* keys = ls.keys();
    uint32_t* vals = ls.vals();      // null when counting
    if (cells != 0) {
        const uint32_t word = count_only ? 0u : 0x80000000u | (uint32_t(fill_mrgb[0]) & 0x7fu) << 24 | uint32_t(fill_mrgb[1]) << 16 |
                                                    uint32_t(fill_mrgb[2]) << 8 | uint32_t(fill_mrgb[3]);
        HIP_TRY(solid_fill(xs.keys(), xs.spare_keys(), pairs, uint32_t(cells), keying, depth, word, keys, vals, s));
    }
    if (hits != 0)
        HIP_TRY(voxelize_emit(f.tq.as<VoxTri>(), f.off.as<uint64_t>(), nt, uint32_t(f.columns), spart.as<uint64_t>(), depth,
                              reinterpret_cast<const uint8_t*>(tri_mrgb), keys + cells, vals ? vals + cells : nullptr, s));
    ScratchBuffer words;
    size_t m = 0;
    if (int rc = sort_unique_list(&ls, uint32_t(entries), depth, &words, s, who, &m)) return rc;
    return voxelize_output(who, ls.keys(), words.as<int32_t>(), m, depth, pos, mrgb, cap, s, n);
} VXRT_CATCH

}  // extern "C"
