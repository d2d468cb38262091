// vxrt.hpp — C++17 host-side mirror of the reference's render-loop types over the C ABI (vxrt.h).
//
// The reference's host is Rust (src/main.rs, src/context.rs, src/camera.rs); no Rust toolchain exists in the build
// image, so the compiled-language host above the C ABI is this header: the same names and argument meaning —
//   Camera{position, direction, fov}                         src/camera.rs:5-9
//   Uniforms / TemporalUniforms / DenoiseUniforms            src/context.rs:425-525, 304-325
//   Context::new / resize / recreate_octree / render         src/context.rs:595-660, 1430-1461, 799-810, 2004-2075
// Errors are reported as vxrt::Error exceptions carrying the vxrt_status and the library's message, where the
// reference returns anyhow::Error (or panics).  Header-only; link with -lvxrt.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "vxrt.h"
#include "vxrt_compact.h"
#include "vxrt_components.h"
#include "vxrt_device_edit.h"
#include "vxrt_device_scene.h"
#include "vxrt_distance.h"
#include "vxrt_edit.h"
#include "vxrt_extract.h"
#include "vxrt_grid.h"
#include "vxrt_grid_edit.h"
#include "vxrt_host.h"
#include "vxrt_pieces.h"
#include "vxrt_query.h"
#include "vxrt_scene_depth.h"
#include "vxrt_setops.h"
#include "vxrt_shape.h"
#include "vxrt_mesh.h"
#include "vxrt_morph.h"
#include "vxrt_solid.h"
#include "vxrt_transform.h"
#include "vxrt_voxelize.h"

namespace vxrt {

class Error : public std::runtime_error {
  public:
    Error(int status, const std::string& where)
        : std::runtime_error(where + ": " + vxrt_status_string(status) + " (" + vxrt_last_error() + ")"), status_(status) {}
    int status() const { return status_; }

  private:
    int status_;
};

inline void check(int status, const char* where) {
    if (status != VXRT_OK) throw Error(status, where);
}

using Vec3 = std::array<float, 3>;

// src/camera.rs:5-9; the default is the reference's start camera (src/context.rs:618-622), fov = 70 degrees.
struct Camera {
    Vec3 position{0.0f, 0.0f, -2.0f};
    Vec3 direction{0.0f, 0.0f, 1.0f};
    float fov = 70.0f * (3.14159274f / 180.0f);

    // Camera::axis_scaled (src/camera.rs:19-28): right, up, forward_ray
    std::array<Vec3, 3> axis_scaled(uint32_t width, uint32_t height) const {
        std::array<Vec3, 3> out{};
        check(vxrt_camera_axis_scaled(position.data(), direction.data(), fov, width, height, out[0].data(), out[1].data(), out[2].data()),
              "vxrt_camera_axis_scaled");
        return out;
    }
};

struct Uniforms : vxrt_uniforms {
    Uniforms() { vxrt_default_uniforms(this); }   // Uniforms::default(), src/context.rs:471-498
};
struct TemporalUniforms : vxrt_temporal {
    TemporalUniforms() { vxrt_default_temporal(this); }
};
struct DenoiseUniforms : vxrt_denoise {
    DenoiseUniforms() { vxrt_default_denoise(this); }
};

// A voxel as the reference's adapters produce it: ([i16; 3], [material, r, g, b]) (src/context.rs:777, 913-933).
struct VoxelList {
    std::vector<std::array<int16_t, 3>> pos;
    std::vector<std::array<uint8_t, 4>> mrgb;
    std::array<uint32_t, 3> size{};
};

// vox::parse + Context::voxels_from_vox (src/vox.rs:11-70, src/context.rs:913-933)
inline VoxelList voxels_from_vox(const std::vector<uint8_t>& bytes) {
    VoxelList v;
    size_t n = 0;
    check(vxrt_vox_to_voxels(bytes.data(), bytes.size(), nullptr, nullptr, 0, &n, v.size.data()), "vxrt_vox_to_voxels");
    v.pos.resize(n);
    v.mrgb.resize(n);
    check(vxrt_vox_to_voxels(bytes.data(), bytes.size(), reinterpret_cast<int16_t(*)[3]>(v.pos.data()),
                             reinterpret_cast<uint8_t(*)[4]>(v.mrgb.data()), n, &n, v.size.data()),
          "vxrt_vox_to_voxels");
    return v;
}

// Whole MagicaVoxel scenes: every shape instance of the scene graph (flags: VXRT_VOX_*, see vxrt.h).
inline VoxelList voxels_from_vox_scene(const std::vector<uint8_t>& bytes, uint32_t flags = VXRT_VOX_ALL_MODELS) {
    VoxelList v;
    size_t n = 0;
    check(vxrt_vox_scene_to_voxels(bytes.data(), bytes.size(), flags, nullptr, nullptr, 0, &n, nullptr, nullptr), "vxrt_vox_scene_to_voxels");
    v.pos.resize(n);
    v.mrgb.resize(n);
    check(vxrt_vox_scene_to_voxels(bytes.data(), bytes.size(), flags, reinterpret_cast<int16_t(*)[3]>(v.pos.data()),
                                   reinterpret_cast<uint8_t(*)[4]>(v.mrgb.data()), n, &n, nullptr, nullptr),
          "vxrt_vox_scene_to_voxels");
    return v;
}

// Context::create_voxels (src/context.rs:838-910): the scene the reference starts with, seeded.
inline VoxelList create_voxels(uint32_t seed = 1) {
    VoxelList v;
    size_t n = 0;
    check(vxrt_default_scene_voxels(seed, nullptr, nullptr, 0, &n), "vxrt_default_scene_voxels");
    v.pos.resize(n);
    v.mrgb.resize(n);
    check(vxrt_default_scene_voxels(seed, reinterpret_cast<int16_t(*)[3]>(v.pos.data()), reinterpret_cast<uint8_t(*)[4]>(v.mrgb.data()), n, &n),
          "vxrt_default_scene_voxels");
    return v;
}

// Context::load_blue_noise (src/context.rs:1042-1085): (image size, all images' pixels appended).
inline std::pair<uint32_t, std::vector<float>> load_blue_noise(const std::string& path) {
    uint32_t size = 0, layers = 0;
    check(vxrt_noise_zip_read(path.c_str(), nullptr, 0, &size, &layers), "vxrt_noise_zip_read");
    std::vector<float> px(size_t(layers) * size * size);
    check(vxrt_noise_zip_read(path.c_str(), px.data(), px.size(), &size, &layers), "vxrt_noise_zip_read");
    return {size, std::move(px)};
}

class Context {
  public:
    Camera camera;
    Uniforms uniforms;
    TemporalUniforms temporal_uniforms;
    DenoiseUniforms denoise_uniforms;

    Context(uint32_t width, uint32_t height, uint32_t max_bounces = 3, int device = 0, uint32_t frames_in_flight = 1,
            uint32_t rank = 0, uint32_t nranks = 1, uint32_t frames_per_launch = 1, uint32_t band_rows = 16)
        : width_(width), height_(height) {
        vxrt_config cfg{};
        cfg.width = width; cfg.height = height; cfg.device = device; cfg.max_bounces = max_bounces;
        cfg.noise_seed = 0x5EED0001u; cfg.noise = nullptr; cfg.rank = rank; cfg.nranks = nranks; cfg.band_rows = band_rows;
        cfg.frames_in_flight = frames_in_flight; cfg.tracer = 0; cfg.frames_per_launch = frames_per_launch;
        check(vxrt_create(&cfg, &ctx_), "vxrt_create");
    }
    ~Context() { vxrt_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;

    // Context::recreate_octree (src/context.rs:799-810)
    void recreate_octree(const VoxelList& voxels) {
        check(vxrt_set_voxels(ctx_, reinterpret_cast<const int16_t(*)[3]>(voxels.pos.data()),
                              reinterpret_cast<const uint8_t(*)[4]>(voxels.mrgb.data()), voxels.pos.size()),
              "vxrt_set_voxels");
    }
    void load_vox(const std::string& path) { check(vxrt_load_vox(ctx_, path.c_str()), "vxrt_load_vox"); }
    // Context::create_blue_noise_buffer (src/context.rs:1016-1040): the archive must hold 128x128 images, 512 of them
    // (BLUE_NOISE_SIZE, and the table length shaders/voxels.comp:65-71 indexes).
    void load_blue_noise(const std::string& path) {
        auto [size, px] = vxrt::load_blue_noise(path);
        if (size != 128 || px.size() != size_t(512) * 128 * 128) throw Error(VXRT_E_NOISE, "blue noise images must be 512 x 128 x 128");
        check(vxrt_set_noise(ctx_, px.data()), "vxrt_set_noise");
    }
    // Makes the table the reference's repository does not ship, on the GPU (include/vxrt_bluenoise.h).
    void generate_blue_noise(uint32_t seed = 0x5EED0001u, int device = 0) {
        std::vector<float> table(size_t(512) * 128 * 128);
        check(vxrt_blue_noise(device, seed, 128, 0, 512, table.data()), "vxrt_blue_noise");
        check(vxrt_set_noise(ctx_, table.data()), "vxrt_set_noise");
    }
    // in-place scene edits (vxrt_edit.h): set / overwrite voxels, clear voxels (absent ones are ignored); the depth never changes.
    // Multi-GPU: every rank holds the whole scene, so the same edits go to every rank's context.
    void edit_voxels(const VoxelList& voxels) {
        if (voxels.mrgb.size() != voxels.pos.size()) throw Error(VXRT_E_INVALID, "edit_voxels: one mrgb per position");
        check(vxrt_edit_voxels(ctx_, reinterpret_cast<const int16_t(*)[3]>(voxels.pos.data()),
                               reinterpret_cast<const uint8_t(*)[4]>(voxels.mrgb.data()), voxels.pos.size()),
              "vxrt_edit_voxels");
    }
    void clear_voxels(const std::vector<std::array<int16_t, 3>>& pos) {
        check(vxrt_edit_voxels(ctx_, reinterpret_cast<const int16_t(*)[3]>(pos.data()), nullptr, pos.size()), "vxrt_edit_voxels");
    }
    // the voxel each ray hits (vxrt_pick_hit: status, time, normal, voxel, leaf word)
    std::vector<vxrt_pick_hit> pick(const std::vector<std::array<float, 3>>& origins, const std::vector<std::array<float, 3>>& dirs) {
        if (origins.size() != dirs.size()) throw Error(VXRT_E_INVALID, "pick: one direction per origin");
        std::vector<vxrt_pick_hit> out(origins.size());
        check(vxrt_pick(ctx_, reinterpret_cast<const float(*)[3]>(origins.data()), reinterpret_cast<const float(*)[3]>(dirs.data()),
                        origins.size(), out.data()),
              "vxrt_pick");
        return out;
    }
    // the scene's voxels (vxrt_extract.h), in octree path order, whole (no box) or those in the half-open box [box_min, box_max);
    // what set_voxels / recreate_octree turns back into the same scene.  size stays 0.
    VoxelList get_voxels() { return get_voxels_in(nullptr, nullptr); }
    VoxelList get_voxels(const std::array<int32_t, 3>& box_min, const std::array<int32_t, 3>& box_max) {
        return get_voxels_in(box_min.data(), box_max.data());
    }
    size_t count_voxels() { return count_in(nullptr, nullptr); }
    size_t count_voxels(const std::array<int32_t, 3>& box_min, const std::array<int32_t, 3>& box_max) {
        return count_in(box_min.data(), box_max.data());
    }
    // vxrt_set_voxels_device (vxrt_device_scene.h): pos / mrgb are n entries in device memory of the context's device, read on the
    // context's stream (a producer on another stream calls context_wait_stream first); the octree is built on the device
    void set_voxels_device(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n) {
        check(vxrt_set_voxels_device(ctx_, pos, mrgb, n), "vxrt_set_voxels_device");
    }
    // vxrt_device_edit.h: edit_voxels / clear_voxels / get_voxels with the lists in device memory of the context's device, read and
    // written on the context's stream.  get_voxels_device: nullptr arrays count; otherwise cap is their room, and the count returns
    void edit_voxels_device(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n) {
        check(vxrt_edit_voxels_device(ctx_, pos, mrgb, n), "vxrt_edit_voxels_device");
    }
    void clear_voxels_device(const int16_t (*pos)[3], size_t n) { check(vxrt_edit_voxels_device(ctx_, pos, nullptr, n), "vxrt_edit_voxels_device"); }
    size_t get_voxels_device(const int32_t* box_min, const int32_t* box_max, int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap) {
        size_t n = 0;
        check(vxrt_get_voxels_device(ctx_, box_min, box_max, pos, mrgb, cap, &n), "vxrt_get_voxels_device");
        return n;
    }
    // vxrt_voxelize.h: the voxels a triangle mesh's surface meets, mesh and list in device memory of the context's device.  nullptr
    // pos / mrgb count; otherwise cap is their room, and the count returns.  The list is what set_voxels_device / edit_voxels_device take
    size_t voxelize_mesh_device(const float (*verts)[3], size_t n_verts, const uint32_t (*tris)[3], const uint8_t (*tri_mrgb)[4], size_t n_tris,
                                int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap) {
        size_t n = 0;
        check(vxrt_voxelize_mesh_device(ctx_, verts, n_verts, tris, tri_mrgb, n_tris, pos, mrgb, cap, &n), "vxrt_voxelize_mesh_device");
        return n;
    }
    // vxrt_solid.h: the interior of a closed mesh (VXRT_SOLID_INTERIOR) or its surface and interior (VXRT_SOLID_UNION), as above;
    // fill_mrgb is host memory
    size_t voxelize_solid_device(const float (*verts)[3], size_t n_verts, const uint32_t (*tris)[3], const uint8_t (*tri_mrgb)[4], size_t n_tris,
                                 const uint8_t fill_mrgb[4], vxrt_solid_mode mode, int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap) {
        size_t n = 0;
        check(vxrt_voxelize_solid_device(ctx_, verts, n_verts, tris, tri_mrgb, n_tris, fill_mrgb, uint32_t(mode), pos, mrgb, cap, &n),
              "vxrt_voxelize_solid_device");
        return n;
    }
    // vxrt_components.h: the connected components of a voxel list in device memory (connectivity 6, 18 or 26): label[i] = the least
    // index of an entry in i's component (nullptr: count only); returns the number of components
    size_t label_components_device(const int16_t (*pos)[3], size_t n, uint32_t connectivity, uint32_t* label) {
        size_t components = 0;
        check(vxrt_label_components_device(ctx_, pos, n, connectivity, label, &components), "vxrt_label_components_device");
        return components;
    }
    // ... and the scene's voxels whose component holds no voxel in the anchor box, as get_voxels_device gives its list; what
    // clear_voxels_device takes to drop them
    size_t detached_voxels_device(const std::array<int32_t, 3>& anchor_min, const std::array<int32_t, 3>& anchor_max, uint32_t connectivity,
                                  int16_t (*pos)[3], uint8_t (*mrgb)[4], size_t cap) {
        size_t n = 0;
        check(vxrt_detached_voxels_device(ctx_, anchor_min.data(), anchor_max.data(), connectivity, pos, mrgb, cap, &n), "vxrt_detached_voxels_device");
        return n;
    }
    // vxrt_pieces.h: the table of a list's components: label and id per entry, info per component (each may be nullptr; info has
    // room for info_cap entries); returns the number of components
    size_t component_table_device(const int16_t (*pos)[3], size_t n, uint32_t connectivity, uint32_t* label, uint32_t* id, vxrt_piece* info,
                                  size_t info_cap) {
        size_t components = 0;
        check(vxrt_component_table_device(ctx_, pos, n, connectivity, label, id, info, info_cap, &components), "vxrt_component_table_device");
        return components;
    }
    // ... and the scene's detached pieces of min_voxels .. max_voxels voxels: their voxels as detached_voxels_device gives them, each
    // one's piece number, and info per piece; returns {voxels, pieces}
    std::pair<size_t, size_t> detached_pieces_device(const std::array<int32_t, 3>& anchor_min, const std::array<int32_t, 3>& anchor_max,
                                                     uint32_t connectivity, uint32_t min_voxels, uint32_t max_voxels, int16_t (*pos)[3],
                                                     uint8_t (*mrgb)[4], uint32_t* piece, size_t cap, vxrt_piece* info, size_t info_cap) {
        size_t n = 0, pieces = 0;
        check(vxrt_detached_pieces_device(ctx_, anchor_min.data(), anchor_max.data(), connectivity, min_voxels, max_voxels, pos, mrgb, piece, cap, &n,
                                          info, info_cap, &pieces),
              "vxrt_detached_pieces_device");
        return {n, pieces};
    }
    // vxrt_query.h: the scene's leaf word at pos[i] + offset per entry (0: no voxel there, or outside the root cube), everything in
    // device memory; leaf == nullptr counts only (the collision test).  Returns the number of nonzero answers.
    size_t lookup_voxels_device(const int16_t (*pos)[3], size_t n, const std::array<int32_t, 3>& offset, uint32_t* leaf) {
        size_t present = 0;
        check(vxrt_lookup_voxels_device(ctx_, pos, n, offset.data(), leaf, &present), "vxrt_lookup_voxels_device");
        return present;
    }
    // ... and pick with rays and hits in device memory, each ray bounded by max_time[i] (nullptr: unbounded, the bytes of pick)
    void pick_device(const float (*origins)[3], const float (*dirs)[3], const float* max_time, size_t n, vxrt_pick_hit* out) {
        check(vxrt_pick_device(ctx_, origins, dirs, max_time, n, out), "vxrt_pick_device");
    }
    // vxrt_transform.h: the list pos / mrgb (device memory; mrgb == nullptr: positions only) resampled under the pull map into the
    // half-open box, in path order.  out_pos == out_mrgb == nullptr counts only.  Returns the number of voxels of the result.
    size_t transform_voxels_device(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, const vxrt_affine& pull,
                                   const std::array<int32_t, 3>& box_min, const std::array<int32_t, 3>& box_max,
                                   int16_t (*out_pos)[3] = nullptr, uint8_t (*out_mrgb)[4] = nullptr, size_t cap = 0) {
        size_t count = 0;
        check(vxrt_transform_voxels_device(ctx_, pos, mrgb, n, &pull, box_min.data(), box_max.data(), out_pos, out_mrgb, cap, &count),
              "vxrt_transform_voxels_device");
        return count;
    }
    // vxrt_shape.h: the cells of the half-open box whose centres the pull map takes into the shape, as a list in device memory in
    // path order; mrgb (host memory, 4 bytes) == nullptr: positions only.  This form counts only.  Returns the number of voxels.
    size_t shape_voxels_device(const vxrt_shape& shape, const vxrt_affine& pull, const std::array<int32_t, 3>& box_min,
                               const std::array<int32_t, 3>& box_max) {
        size_t count = 0;
        check(vxrt_shape_voxels_device(ctx_, &shape, &pull, box_min.data(), box_max.data(), nullptr, nullptr, nullptr, 0, &count),
              "vxrt_shape_voxels_device");
        return count;
    }
    // ... and this one writes out_pos and, with mrgb, out_mrgb, which have room for cap voxels.
    size_t shape_voxels_device(const vxrt_shape& shape, const vxrt_affine& pull, const std::array<int32_t, 3>& box_min,
                               const std::array<int32_t, 3>& box_max, const uint8_t* mrgb, int16_t (*out_pos)[3], uint8_t (*out_mrgb)[4],
                               size_t cap) {
        size_t count = 0;
        check(vxrt_shape_voxels_device(ctx_, &shape, &pull, box_min.data(), box_max.data(), mrgb, out_pos, out_mrgb, cap, &count),
              "vxrt_shape_voxels_device");
        return count;
    }
    // vxrt_setops.h: the lists A and B (device memory; a_mrgb == nullptr: positions only) combined under op, in path order.
    // out_pos == out_mrgb == nullptr counts only.  Returns the number of voxels of the result.
    size_t combine_voxels_device(const int16_t (*a_pos)[3], const uint8_t (*a_mrgb)[4], size_t na, const int16_t (*b_pos)[3],
                                 const uint8_t (*b_mrgb)[4], size_t nb, vxrt_list_op op, int16_t (*out_pos)[3] = nullptr,
                                 uint8_t (*out_mrgb)[4] = nullptr, size_t cap = 0) {
        size_t count = 0;
        check(vxrt_combine_voxels_device(ctx_, a_pos, a_mrgb, na, b_pos, b_mrgb, nb, uint32_t(op), out_pos, out_mrgb, cap, &count),
              "vxrt_combine_voxels_device");
        return count;
    }
    // vxrt_morph.h: the list (device memory; mrgb == nullptr: positions only) dilated, eroded, or its surface layer or margin ring,
    // under the 6, 18 or 26 neighbourhood, `steps` cells deep, in path order.  out_pos == out_mrgb == nullptr counts only.  Returns
    // the number of voxels of the result.
    size_t morph_voxels_device(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, vxrt_morph_op op, uint32_t connectivity = 6,
                               uint32_t steps = 1, int16_t (*out_pos)[3] = nullptr, uint8_t (*out_mrgb)[4] = nullptr, size_t cap = 0) {
        size_t count = 0;
        check(vxrt_morph_voxels_device(ctx_, pos, mrgb, n, uint32_t(op), connectivity, steps, out_pos, out_mrgb, cap, &count),
              "vxrt_morph_voxels_device");
        return count;
    }
    // vxrt_distance.h: the list's exact squared Euclidean distance transform (device memory; mrgb == nullptr: positions only): every
    // voxel's d2 to the nearest empty cell (VXRT_DISTANCE_DEPTH), every empty cell within max_d2 of a voxel (VXRT_DISTANCE_FIELD), or
    // the list eroded / dilated by the ball of squared radius max_d2, in path order.  out_pos == nullptr counts only.  Returns the
    // number of voxels of the result.
    size_t distance_voxels_device(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, vxrt_distance_mode mode, uint32_t max_d2,
                                  int16_t (*out_pos)[3] = nullptr, uint8_t (*out_mrgb)[4] = nullptr, uint16_t* out_d2 = nullptr, size_t cap = 0) {
        size_t count = 0;
        check(vxrt_distance_voxels_device(ctx_, pos, mrgb, n, uint32_t(mode), max_d2, out_pos, out_mrgb, out_d2, cap, &count),
              "vxrt_distance_voxels_device");
        return count;
    }
    // vxrt_mesh.h: the list's exposed faces (device memory; mrgb == nullptr: positions only) as an indexed triangle mesh, one quad
    // per face (VXRT_MESH_FACES) or per run of faces of one row and colour (VXRT_MESH_RUNS).  out_verts == out_tris == nullptr
    // counts only.  Returns {vertices, triangles}.
    std::pair<size_t, size_t> mesh_voxels_device(const int16_t (*pos)[3], const uint8_t (*mrgb)[4], size_t n, vxrt_mesh_mode mode = VXRT_MESH_RUNS,
                                                 float (*out_verts)[3] = nullptr, size_t vert_cap = 0, uint32_t (*out_tris)[3] = nullptr,
                                                 uint8_t (*out_tri_mrgb)[4] = nullptr, size_t tri_cap = 0) {
        size_t verts = 0, tris = 0;
        check(vxrt_mesh_voxels_device(ctx_, pos, mrgb, n, uint32_t(mode), out_verts, vert_cap, out_tris, out_tri_mrgb, tri_cap, &verts, &tris),
              "vxrt_mesh_voxels_device");
        return {verts, tris};
    }
    // vxrt_set_voxel_grid (vxrt_grid.h): dims[0] x dims[1] x dims[2] cells in device memory of the context's device, C order
    // [x][y][z], cell (i, j, k) at origin + (i, j, k); palette: 256 entries for VXRT_GRID_PALETTE8, nullptr for VXRT_GRID_WORD32
    void set_voxel_grid(const void* cells, vxrt_grid_format format, const std::array<uint32_t, 3>& dims,
                        const std::array<int32_t, 3>& origin = {0, 0, 0}, const uint8_t (*palette)[4] = nullptr) {
        check(vxrt_set_voxel_grid(ctx_, cells, format, dims.data(), origin.data(), palette), "vxrt_set_voxel_grid");
    }
    // vxrt_get_voxel_grid: the box origin + [0, dims) as leaf words into device memory, enqueued on the context's stream (a consumer on
    // another stream calls stream_wait_context first)
    void get_voxel_grid(const std::array<int32_t, 3>& origin, const std::array<uint32_t, 3>& dims, uint32_t* cells) {
        check(vxrt_get_voxel_grid(ctx_, origin.data(), dims.data(), cells), "vxrt_get_voxel_grid");
    }
    // vxrt_edit_voxel_grid (vxrt_grid_edit.h): the grid (as set_voxel_grid takes it) written into the box origin + [0, dims) of the
    // scene in place; returns how many cells were set and cleared
    vxrt_grid_edit_counts edit_voxel_grid(const void* cells, vxrt_grid_format format, const std::array<uint32_t, 3>& dims,
                                          const std::array<int32_t, 3>& origin = {0, 0, 0}, const uint8_t (*palette)[4] = nullptr,
                                          vxrt_grid_edit_mode mode = VXRT_GRID_EDIT_REPLACE) {
        vxrt_grid_edit_counts counts{0, 0};
        check(vxrt_edit_voxel_grid(ctx_, cells, format, dims.data(), origin.data(), palette, mode, &counts), "vxrt_edit_voxel_grid");
        return counts;
    }
    // vxrt_scene_depth.h: the scene's octree depth changed in place (root cube [-2^depth, 2^depth)^3; a shrink that would drop a voxel
    // throws VXRT_E_SCENE), or set to what a rebuild of its voxels would give (returned)
    void set_scene_depth(uint32_t depth) { check(vxrt_set_scene_depth(ctx_, depth), "vxrt_set_scene_depth"); }
    uint32_t fit_scene_depth() {
        uint32_t depth = 0;
        check(vxrt_fit_scene_depth(ctx_, &depth), "vxrt_fit_scene_depth");
        return depth;
    }
    // vxrt_compact.h: the edited scene re-laid as a fresh build of the same tree lies (the holes edits left are given back), and
    // the storage counts a host decides by
    void compact_scene() { check(vxrt_compact_scene(ctx_), "vxrt_compact_scene"); }
    vxrt_scene_storage scene_storage() {
        vxrt_scene_storage s{};
        check(vxrt_get_scene_storage(ctx_, &s), "vxrt_get_scene_storage");
        return s;
    }
    void set_menger(uint32_t level, uint32_t clip, std::array<uint8_t, 4> mrgb, uint32_t emissive_period) {
        check(vxrt_set_menger(ctx_, level, clip, mrgb.data(), emissive_period), "vxrt_set_menger");
    }
    // Context::resize (src/context.rs:1430-1461)
    void resize(uint32_t width, uint32_t height) {
        check(vxrt_resize(ctx_, width, height), "vxrt_resize");
        width_ = width; height_ = height;
    }
    // Context::update_bindings + render (src/context.rs:2136-2162, 2004-2075)
    void render(uint32_t flags = VXRT_ALL) {
        check(vxrt_set_camera(ctx_, camera.position.data(), camera.direction.data(), camera.fov), "vxrt_set_camera");
        check(vxrt_set_scene_params(ctx_, &uniforms), "vxrt_set_scene_params");
        check(vxrt_set_temporal(ctx_, &temporal_uniforms), "vxrt_set_temporal");
        check(vxrt_set_denoise(ctx_, &denoise_uniforms), "vxrt_set_denoise");
        check(vxrt_render(ctx_, flags), "vxrt_render");
    }
    // `count` frames with the camera and parameters at rest (one trace launch per frames_per_launch frames)
    void render_frames(uint32_t flags, uint32_t count) {
        check(vxrt_set_camera(ctx_, camera.position.data(), camera.direction.data(), camera.fov), "vxrt_set_camera");
        check(vxrt_set_scene_params(ctx_, &uniforms), "vxrt_set_scene_params");
        check(vxrt_set_temporal(ctx_, &temporal_uniforms), "vxrt_set_temporal");
        check(vxrt_set_denoise(ctx_, &denoise_uniforms), "vxrt_set_denoise");
        check(vxrt_render_frames(ctx_, flags, count), "vxrt_render_frames");
    }
    // frames along a camera path (vxrt_render_path); `camera` ends at the last pose
    void render_path(uint32_t flags, const std::vector<Vec3>& positions, const std::vector<Vec3>& directions) {
        if (positions.size() != directions.size()) throw Error(VXRT_E_INVALID, "render_path: one direction per position");
        check(vxrt_set_scene_params(ctx_, &uniforms), "vxrt_set_scene_params");
        check(vxrt_set_temporal(ctx_, &temporal_uniforms), "vxrt_set_temporal");
        check(vxrt_set_denoise(ctx_, &denoise_uniforms), "vxrt_set_denoise");
        check(vxrt_render_path(ctx_, flags, uint32_t(positions.size()), reinterpret_cast<const float(*)[3]>(positions.data()),
                               reinterpret_cast<const float(*)[3]>(directions.data()), camera.fov), "vxrt_render_path");
        if (!positions.empty()) { camera.position = positions.back(); camera.direction = directions.back(); }
    }
    // one displayed frame of `spp` samples per pixel (vxrt_render_spp)
    void render_spp(uint32_t flags, uint32_t spp) {
        check(vxrt_set_camera(ctx_, camera.position.data(), camera.direction.data(), camera.fov), "vxrt_set_camera");
        check(vxrt_set_scene_params(ctx_, &uniforms), "vxrt_set_scene_params");
        check(vxrt_set_temporal(ctx_, &temporal_uniforms), "vxrt_set_temporal");
        check(vxrt_set_denoise(ctx_, &denoise_uniforms), "vxrt_set_denoise");
        check(vxrt_render_spp(ctx_, flags, spp), "vxrt_render_spp");
    }
    // vxrt_render without re-pushing the parameter blocks: the stages of a frame around a halo exchange
    void render_stage(uint32_t flags) { check(vxrt_render(ctx_, flags), "vxrt_render"); }
    // Multi-GPU halo (vxrt.h "halo"): one frame of a rank = render(VXRT_TRACE | VXRT_TEMPORAL); halo_pack; [send / receive on comm_stream];
    // render_stage(VXRT_DENOISE_INTERIOR); halo_unpack; render_stage(VXRT_DENOISE_EDGE) — ordered by events, the host never waits.
    vxrt_halo_info halo_info() {
        check(vxrt_set_denoise(ctx_, &denoise_uniforms), "vxrt_set_denoise");   // the halo's row count follows the radius
        vxrt_halo_info info{};
        check(vxrt_halo_info_get(ctx_, &info), "vxrt_halo_info_get");
        return info;
    }
    void halo_pack(void* dev_to_prev, void* dev_to_next, void* comm_stream) {
        check(vxrt_halo_pack(ctx_, dev_to_prev, dev_to_next), "vxrt_halo_pack");
        check(vxrt_stream_wait_context(ctx_, comm_stream), "vxrt_stream_wait_context");
    }
    void halo_unpack(const void* dev_from_prev, const void* dev_from_next, void* comm_stream) {
        check(vxrt_context_wait_stream(ctx_, comm_stream), "vxrt_context_wait_stream");
        check(vxrt_halo_unpack(ctx_, dev_from_prev, dev_from_next), "vxrt_halo_unpack");
    }
    // run-time options (vxrt.h: VXRT_OPT_DENOISE_MODE, VXRT_OPT_TAIL_CAPACITY, VXRT_OPT_SCENE_FORMAT, VXRT_OPT_HALO_ROWS, VXRT_OPT_SKY_CULL)
    void set_option(vxrt_option option, uint32_t value) { check(vxrt_set_option(ctx_, option, value), "vxrt_set_option"); }
    void sync() { check(vxrt_sync(ctx_), "vxrt_sync"); }
    std::vector<float> read(vxrt_image which) {
        uint32_t rows = 0;
        check(vxrt_local_rows(ctx_, &rows, nullptr), "vxrt_local_rows");
        std::vector<float> img(size_t(rows) * width_ * 4);
        check(vxrt_read(ctx_, which, img.data(), img.size() * sizeof(float)), "vxrt_read");
        return img;
    }
    // The displayed frame (VXRT_DISPLAY_BGRA8_SRGB / VXRT_DISPLAY_RGBA8_SRGB): VXRT_DENOISED encoded to 8-bit sRGB on the GPU by the
    // library's exact rule, local rows x width x 4 bytes
    std::vector<uint8_t> read_display(vxrt_image which) {
        std::vector<uint8_t> img(display_bytes());
        check(vxrt_read(ctx_, which, reinterpret_cast<float*>(img.data()), img.size()), "vxrt_read");
        return img;
    }
    // bytes of one display image of this context (its local rows x width x 4)
    size_t display_bytes() const { return image_floats(); }
    // floats of one image of this context (its local rows x width x 4)
    size_t image_floats() const {
        uint32_t rows = 0;
        check(vxrt_local_rows(ctx_, &rows, nullptr), "vxrt_local_rows");
        return size_t(rows) * width_ * 4;
    }
    // The non-blocking read-back (vxrt_read_async / vxrt_read_wait): what a host that shows or stores EVERY frame calls where the
    // reference presents (src/context.rs:2046-2070).  Frame k: render(...); read_async(VXRT_DENOISED, buf[k & 1], k & 1); then
    // read_wait((k + 1) & 1) and frame k - 1 is in buf[(k + 1) & 1] — it travelled while frame k rendered.
    void read_async(vxrt_image which, class PinnedImage& dst, uint32_t slot);
    // ... and of a display image into pinned bytes: a quarter of the rgba32f transfer (read_async(VXRT_DISPLAY_BGRA8_SRGB, buf[k & 1], k & 1))
    void read_async(vxrt_image which, class PinnedDisplay& dst, uint32_t slot);
    void read_wait(uint32_t slot) { check(vxrt_read_wait(ctx_, slot), "vxrt_read_wait"); }
    vxrt_stats stats() {
        vxrt_stats s{};
        check(vxrt_get_stats(ctx_, &s), "vxrt_get_stats");
        return s;
    }
    uint32_t width() const { return width_; }
    uint32_t height() const { return height_; }
    vxrt_ctx* handle() { return ctx_; }

  private:
    size_t count_in(const int32_t* lo, const int32_t* hi) {
        size_t n = 0;
        check(vxrt_get_voxels(ctx_, lo, hi, nullptr, nullptr, 0, &n), "vxrt_get_voxels");
        return n;
    }
    VoxelList get_voxels_in(const int32_t* lo, const int32_t* hi) {
        VoxelList v;
        size_t n = count_in(lo, hi);
        // the scene cannot change between the two calls (edits are calls on this context), so the count is the count
        v.pos.resize(n);
        v.mrgb.resize(n);
        check(vxrt_get_voxels(ctx_, lo, hi, reinterpret_cast<int16_t(*)[3]>(v.pos.data()), reinterpret_cast<uint8_t(*)[4]>(v.mrgb.data()), n, &n),
              "vxrt_get_voxels");
        return v;
    }
    vxrt_ctx* ctx_ = nullptr;
    uint32_t width_, height_;
};

// Pinned host memory for Context::read_async (vxrt_host_alloc / vxrt_host_free): a host needs no HIP binding of its own for it.
class PinnedImage {
  public:
    explicit PinnedImage(size_t floats) : floats_(floats) {
        void* p = nullptr;
        check(vxrt_host_alloc(floats * sizeof(float), &p), "vxrt_host_alloc");
        data_ = static_cast<float*>(p);
    }
    ~PinnedImage() { if (data_) (void)vxrt_host_free(data_); }
    PinnedImage(const PinnedImage&) = delete;
    PinnedImage& operator=(const PinnedImage&) = delete;
    float* data() { return data_; }
    const float* data() const { return data_; }
    size_t size() const { return floats_; }
    size_t bytes() const { return floats_ * sizeof(float); }

  private:
    float* data_ = nullptr;
    size_t floats_;
};

inline void Context::read_async(vxrt_image which, PinnedImage& dst, uint32_t slot) {
    check(vxrt_read_async(ctx_, which, dst.data(), dst.bytes(), slot), "vxrt_read_async");
}

// Pinned host bytes for Context::read_async of a display image (Context::display_bytes() of them).
class PinnedDisplay {
  public:
    explicit PinnedDisplay(size_t bytes) : bytes_(bytes) {
        void* p = nullptr;
        check(vxrt_host_alloc(bytes, &p), "vxrt_host_alloc");
        data_ = static_cast<uint8_t*>(p);
    }
    ~PinnedDisplay() { if (data_) (void)vxrt_host_free(data_); }
    PinnedDisplay(const PinnedDisplay&) = delete;
    PinnedDisplay& operator=(const PinnedDisplay&) = delete;
    uint8_t* data() { return data_; }
    const uint8_t* data() const { return data_; }
    size_t size() const { return bytes_; }
    size_t bytes() const { return bytes_; }

  private:
    uint8_t* data_ = nullptr;
    size_t bytes_;
};

inline void Context::read_async(vxrt_image which, PinnedDisplay& dst, uint32_t slot) {
    // dst receives bytes; the C signature keeps float* (vxrt.h)
    check(vxrt_read_async(ctx_, which, reinterpret_cast<float*>(dst.data()), dst.bytes(), slot), "vxrt_read_async");
}

}  // namespace vxrt
