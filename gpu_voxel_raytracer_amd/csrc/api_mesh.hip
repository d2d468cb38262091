// api_mesh.hip — host side of vxrt_mesh.h: the exposed faces of a voxel list in device memory as an indexed triangle mesh.  The
// list is keyed, sorted and deduplicated by list_ops.h's key_list; morph.hip gives each voxel its 6-neighbour mask; mesh.hip counts
// and writes the faces as sortable keys; the list builder's radix sort puts them in face-key order, where a run is a stretch of
// consecutive keys; the run heads are counted and written, each quad's four corner keys written and sorted (keys only), the
// distinct corners counted and written (list_ops.h's run heads at shift 0); the last two kernels look each quad's corners up and write the caller's arrays.  Nothing
// but counts crosses to the host.  DESIGN.md §27.
#include <string>

#include "list_ops.h"
#include "mesh.h"
#include "scene_args.h"
#include "../../include/vxrt_mesh.h"

namespace vxrt {
namespace {

// An output array of `cap` entries of `each` bytes, 4-byte aligned where `aligned`.
int check_mesh_output(const vxrt_ctx* c, const void* p, size_t cap, size_t each, bool aligned, const char* who, const char* what) {
    if (!p) return VXRT_OK;
    if (aligned && (reinterpret_cast<uintptr_t>(p) & 3u) != 0u) {
        set_error(std::string(who) + ": " + what + " is not 4-byte aligned");
        return VXRT_E_INVALID;
    }
    if (cap > SIZE_MAX / each) {
        set_error(std::string(who) + ": " + what + " ends past its allocation");
        return VXRT_E_INVALID;
    }
    return check_device_array(c, p, cap * each, who, what);
}

}  // namespace
}  // namespace vxrt

extern "C" {

int vxrt_mesh_voxels_device(vxrt_ctx* c, const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, uint32_t mode, float (*out_verts)[3],
                            size_t vert_cap, uint32_t (*out_tris)[3], uint8_t (*out_tri_mrgb)[4], size_t tri_cap, size_t* n_verts,
                            size_t* n_tris) try {
    using namespace vxrt;
    const char* who = "vxrt_mesh_voxels_device";
    const std::string w = who;
    if (!valid_ctx(c)) { set_error("null context"); return VXRT_E_INVALID; }
    if (uint64_t(n) >= (uint64_t(1) << 32)) { set_error(w + ": 2^32 voxels or more"); return VXRT_E_INVALID; }
    if (!n_verts || !n_tris) { set_error(w + (n_verts ? ": null n_tris" : ": null n_verts")); return VXRT_E_INVALID; }
    if (mode > uint32_t(VXRT_MESH_RUNS)) { set_error(w + ": mode is no vxrt_mesh_mode"); return VXRT_E_INVALID; }
    if ((out_verts != nullptr) != (out_tris != nullptr)) { set_error(w + ": out_verts and out_tris come both or neither"); return VXRT_E_INVALID; }
    const bool with_vals = mrgb != nullptr;
    if (!with_vals && out_tri_mrgb) { set_error(w + ": out_tri_mrgb without mrgb"); return VXRT_E_INVALID; }
    if (with_vals && (out_tris != nullptr) != (out_tri_mrgb != nullptr)) {
        set_error(w + ": out_tris and out_tri_mrgb come both or neither");
        return VXRT_E_INVALID;
    }
    if (n != 0 && !pos) { set_error(w + ": null voxel positions"); return VXRT_E_INVALID; }
    if (n == 0) { *n_verts = 0; *n_tris = 0; return VXRT_OK; }

    HIP_TRY(hipSetDevice(c->cfg.device));
    if (int rc = check_input_list(c, pos, mrgb, n, who, "pos", "mrgb")) return rc;
    if (int rc = check_mesh_output(c, out_verts, vert_cap, 3 * sizeof(float), true, who, "out_verts")) return rc;
    if (int rc = check_mesh_output(c, out_tris, tri_cap, 3 * sizeof(uint32_t), true, who, "out_tris")) return rc;
    if (int rc = check_mesh_output(c, out_tri_mrgb, tri_cap, 4, false, who, "out_tri_mrgb")) return rc;

    // the list: sorted, one key per position, the last entry's bytes.  Every input byte is read here, into scratch, before the two
    // kernels at the end write the first output byte.  The leaf words come along where a count depends on them (RUNS: a run ends
    // where the bytes change) or they are written.
    hipStream_t s = c->stream;     // behind everything enqueued there, vxrt_context_wait_stream's events included
    const bool words = with_vals && (mode == uint32_t(VXRT_MESH_RUNS) || out_tris != nullptr);
    KeyedList list;
    if (int rc = key_list(pos, mrgb, n, words, s, who, &list, nullptr)) return rc;
    const MorphSet set = list.view;      // 0 < m <= n

    // the faces: a voxel has one wherever its 6-neighbour mask has no bit
    uint64_t faces = 0;
    KeySort fs;      // the faces, double-buffered for the sort
    {
        ScratchBuffer masks, part;
        if (int rc = alloc_scratch(&masks, size_t(set.m) * sizeof(uint32_t), who, "the neighbour masks")) return rc;
        if (int rc = alloc_part(&part, set.m, who)) return rc;
        HIP_TRY(launch_morph_mask(set, kMeshDirs, kMorphErode, false, masks.as<uint32_t>(), part.as<uint64_t>(), s));
        HIP_TRY(launch_mesh_face_count(masks.as<uint32_t>(), set.m, part.as<uint64_t>(), s));
        if (int rc = scan_total(part.as<uint64_t>(), morph_blocks(set.m), s, &faces)) return rc;
        if (faces >= (uint64_t(1) << 32)) { set_error(w + ": 2^32 faces or more"); return VXRT_E_INVALID; }
        if (faces == 0) { set_error(w + ": internal error: a set without a face"); return VXRT_E_INVALID; }
        if (int rc = fs.alloc(size_t(faces), words, who)) return rc;
        HIP_TRY(launch_mesh_face_emit(set, masks.as<uint32_t>(), part.as<uint64_t>(), fs.keys(), fs.vals(), s));
        HIP_TRY(fs.sort(uint32_t(faces), kMeshFaceBits, s));
        HIP_TRY(hipStreamSynchronize(s));      // masks and part are freed here
    }
    const uint64_t* sorted_faces = fs.keys();
    const uint32_t* sorted_words = fs.vals();      // null without words

    // the quads: one per run head
    uint64_t quads = 0;
    ScratchBuffer heads, hpart;
    if (int rc = alloc_part(&hpart, faces, who)) return rc;
    HIP_TRY(launch_mesh_heads(sorted_faces, sorted_words, uint32_t(faces), mode, hpart.as<uint64_t>(), nullptr, s));
    if (int rc = scan_total(hpart.as<uint64_t>(), morph_blocks(faces), s, &quads)) return rc;
    if (4 * quads >= (uint64_t(1) << 32)) { set_error(w + ": 2^30 quads or more"); return VXRT_E_INVALID; }
    if (quads == 0) { set_error(w + ": internal error: faces without a quad"); return VXRT_E_INVALID; }
    if (int rc = alloc_scratch(&heads, size_t(quads) * sizeof(uint32_t), who, "the run heads")) return rc;
    HIP_TRY(launch_mesh_heads(sorted_faces, sorted_words, uint32_t(faces), mode, hpart.as<uint64_t>(), heads.as<uint32_t>(), s));

    // the vertices: the distinct corners of all quads, ascending by (x, y, z)
    const uint32_t corners = uint32_t(4 * quads);
    KeySort cs;
    ScratchBuffer verts;
    if (int rc = cs.alloc(size_t(corners), false, who)) return rc;
    HIP_TRY(launch_mesh_quad_corners(sorted_faces, uint32_t(faces), heads.as<uint32_t>(), uint32_t(quads), cs.keys(), s));
    HIP_TRY(cs.sort(corners, kMeshCornerBits, s));
    RunHeads firsts;
    if (int rc = run_heads_count(cs.keys(), corners, 0u, s, who, &firsts)) return rc;
    const uint64_t distinct = firsts.count;

    // the caps
    *n_verts = size_t(distinct);
    *n_tris = size_t(2 * quads);
    if (!out_verts) return VXRT_OK;
    if (distinct > vert_cap || 2 * quads > tri_cap) {
        set_error(w + ": " + std::to_string(distinct) + " vertices and " + std::to_string(2 * quads) + " triangles, room for " +
                  std::to_string(vert_cap) + " and " + std::to_string(tri_cap));
        return VXRT_E_INVALID;
    }
    if (int rc = alloc_scratch(&verts, size_t(distinct) * sizeof(uint64_t), who, "the vertices")) return rc;
    if (int rc = run_heads_emit(firsts, nullptr, verts.as<uint64_t>(), nullptr, s)) return rc;

    // the only kernels that write an output byte
    HIP_TRY(launch_mesh_triangles(sorted_faces, sorted_words, uint32_t(faces), heads.as<uint32_t>(), uint32_t(quads), verts.as<uint64_t>(),
                                  uint32_t(distinct), reinterpret_cast<uint32_t*>(out_tris), reinterpret_cast<uint8_t*>(out_tri_mrgb), s));
    HIP_TRY(launch_mesh_vertices(verts.as<uint64_t>(), uint32_t(distinct), reinterpret_cast<float*>(out_verts), s));
    HIP_TRY(hipStreamSynchronize(s));
    return VXRT_OK;
} VXRT_CATCH

}  // extern "C"
