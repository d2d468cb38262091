// device_build.h — what api_device_scene.hip (host side of vxrt_device_scene.h) and device_build.hip (the builder) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

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
    size_t scratch_bytes = 0;   // the build's peak scratch (freed before it returns)
};

// pos / mrgb: n entries in device memory of the current device, read on `stream` behind what is enqueued there.  Waits for the
// result.  VXRT_E_SCENE: depth > 15 or 2^32 records or more; VXRT_E_DEVICE: an allocation or launch failed.  Nothing is allocated
// on failure.  The pipeline is in device_build.hip and DESIGN.md §11.
int build_svo_device_list(const int16_t* pos, const uint8_t* mrgb, size_t n, hipStream_t stream, DeviceTree* out);

}  // namespace vxrt
