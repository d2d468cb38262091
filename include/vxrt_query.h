/*
 * vxrt_query.h — questions about the loaded scene asked and answered in device memory: is the scene occupied at these positions, and
 * what does this ray hit within this distance.  The optional extension of libvxrt.so for hosts that move what they broke off: the
 * collision test of a piece (vxrt_pieces.h) at a trial displacement, a swept particle, line of sight, a landing test along gravity,
 * a brush or a mask that samples the scene.  It is the read side of vxrt_device_edit.h: detach, move, test and re-insert without a
 * round trip through the host.  A host that only renders needs nothing from here.  Conventions as in vxrt.h: 0 or a negative
 * vxrt_status.
 *
 * The lookup rule is exact and does not depend on schedule, device or call:
 *   1. q = pos[i] + offset per axis, taken without wrap (offset may be INT32_MIN or INT32_MAX; offset == NULL is zero)
 *   2. q outside the scene's root cube [-2^d, 2^d)^3, d = vxrt_stats.octree_depth: the answer is 0 — not an error, a piece under
 *      test may stick out of the cube
 *   3. otherwise the answer is the voxel's leaf word as vxrt_pick reports it (0x80000000 | (material & 0x7f) << 24 | rgb), or 0
 *      where the scene has no voxel at q
 *   4. *n_present is the number of i with a nonzero answer; a position listed twice counts twice
 *
 * The ray rule: status, time, normal and leaf are those of the shader's cast_bounded_ray with max_distance = max_time[i], computed
 * by the code the tracers run; voxel is vxrt_pick's (vxrt_edit.h).  max_time == NULL casts every ray unbounded, and out is then
 * byte for byte what vxrt_pick writes for the same rays; a max_time[i] of 2^30 (the shader's ALMOST_INFINITY) is the same as
 * unbounded; every other value — 0, negatives and NaN included — is the shader's own comparison.  Non-finite origins and
 * directions behave as vxrt_pick documents.
 *
 * Both calls read scenes in any record order (breadth first, edited with holes, compacted, VXRT_OPT_NODE_ORDER 2 / 3): they follow
 * the 8-byte records from the root, as vxrt_pick and vxrt_get_voxels_device do.  They change no scene byte, image, history or stat.
 *
 * Ordering: the arrays are read and written on the context's stream, behind everything enqueued there; a producer on another stream
 * orders itself first with vxrt_context_wait_stream(ctx, producer_stream).  Unlike vxrt_pick the calls do not wait for the context's
 * other work first; they wait for their own result, so the arrays may be freed or rewritten when they return.  Two calls with the
 * same arguments write the same bytes.
 *
 * Multi-GPU: every rank holds the whole scene; ask each rank's context, in its own device's memory.
 */
#ifndef VXRT_QUERY_H
#define VXRT_QUERY_H

#include "vxrt.h"
#include "vxrt_edit.h"

#ifdef __cplusplus
extern "C" {
#endif

/* pos[0 .. n) and leaf[0 .. n) are device memory of the context's device; leaf is 4-byte aligned, pos may have any alignment and is
 * never written.  leaf and n_present are each optional: leaf == NULL only counts (the collision test), n_present == NULL only
 * writes the words.  Scratch, freed before the call returns: one count per 2 048 entries.
 *
 * Checked in this order:
 *   VXRT_E_INVALID  null context; n >= 2^32 (before any pointer is looked at)
 *   n == 0          returns 0 without touching a pointer, after setting *n_present = 0 where that is given
 *   VXRT_E_INVALID  null pos; leaf and n_present both null; a misaligned leaf; an array that hipPointerGetAttributes does not report
 *                   as device memory of the context's device, or that ends past its allocation
 *   VXRT_E_NOSCENE  no scene is loaded
 *   VXRT_E_SCENE    a scene deeper than 15 (no call of this library builds one: int16 positions end at depth 15)
 *   VXRT_E_DEVICE   the scratch could not be allocated
 * A refused call writes nothing. */
int vxrt_lookup_voxels_device(vxrt_ctx* ctx, const int16_t (*pos)[3], size_t n, const int32_t offset[3], uint32_t* leaf,
                              size_t* n_present);

/* origins[0 .. n), dirs[0 .. n), max_time[0 .. n) (or NULL: unbounded) and out[0 .. n) are device memory of the context's device,
 * each 4-byte aligned; world units as the tracers cast them.  Allocates nothing.
 *
 * Checked in this order:
 *   VXRT_E_INVALID  null context; n >= 2^31 (before any pointer is looked at)
 *   n == 0          returns 0 without touching a pointer
 *   VXRT_E_INVALID  null origins, dirs or out; a misaligned array; an array that is not device memory of the context's device, or
 *                   that ends past its allocation
 *   VXRT_E_NOSCENE  no scene is loaded
 * A refused call writes nothing. */
int vxrt_pick_device(vxrt_ctx* ctx, const float (*origins)[3], const float (*dirs)[3], const float* max_time, size_t n,
                     vxrt_pick_hit* out);

#ifdef __cplusplus
}
#endif

#endif /* VXRT_QUERY_H */
