// pieces.h — what api_pieces.hip (host side of vxrt_pieces.h) and pieces.hip (its kernels) share.  They run behind a labelling
// (components.h: label_list) and read what it leaves.  DESIGN.md §21.
#pragma once
#include "components.h"
#include "../../include/vxrt_pieces.h"

namespace vxrt {

// One component's accumulators; k of them, indexed by the root's rank among the roots in key order (its "slot").  Coordinates are
// biased, u = p + 32768, so minima and maxima are unsigned; the bias leaves the sums at emit.
struct PieceAcc {
    unsigned long long sum[3];   // of u over the distinct positions
    uint32_t count;              // distinct positions
    uint32_t first;              // the least input index of an entry in the component: its label
    uint32_t lo[3], hi[3];       // of u
    uint32_t id;                 // slots: kPieceHeld or kCompNone; mark: kCompNone unless selected; number: a selected one's number
    uint32_t start;              // the scene call: the index in the returned list of the component's first voxel
};
static_assert(sizeof(PieceAcc) == 64, "PieceAcc");
constexpr uint32_t kPieceHeld = 0xfffffffeu;   // a component with a voxel in the anchor box

// Over the m unique voxels, part = the flatten's scanned root counts: a root x gets slot[x] = its rank among the roots, and its
// accumulators their start values; id = kPieceHeld where anchored != 0 and acc[x] == 0, kCompNone otherwise.
hipError_t pieces_slots(const uint32_t* comp, const uint32_t* acc, uint32_t m, const uint64_t* part, uint32_t anchored, uint32_t* slot,
                        PieceAcc* accs, hipStream_t s);

// Over the m unique voxels in key order: count, first, lo, hi and sum per component, each run of equal roots reduced inside its wave
// and added by the run's last lane.
hipError_t pieces_reduce(const uint64_t* ukeys, const uint32_t* uhead, const uint32_t* comp, const uint32_t* slot, uint32_t m, PieceAcc* accs,
                         hipStream_t s);

// One thread per component: where it is not held and min_voxels <= count <= max_voxels, mark[first] = slot + 1 (mark: n words,
// zeroed); id = kCompNone where it is not selected.
hipError_t pieces_mark(PieceAcc* accs, uint32_t k, uint32_t n, uint32_t min_voxels, uint32_t max_voxels, uint32_t* mark, hipStream_t s);

// Over the n sorted entries: pick[sorted[i]] = slot + 1 of the entry's component where that is selected, else 0.
hipError_t pieces_pick(const uint32_t* sorted, const uint32_t* rank, uint32_t n, const uint32_t* comp, const uint32_t* slot, const PieceAcc* accs,
                       uint32_t* pick, hipStream_t s);

// mark_part = components_select_count(mark) scanned.  Over the n input indices: the component marked at i gets id = the marks before
// i, and with pick (pick_part = its scanned counts) start = the picked entries before i.
hipError_t pieces_number(const uint32_t* mark, uint32_t n, const uint64_t* mark_part, const uint32_t* pick, const uint64_t* pick_part,
                         PieceAcc* accs, hipStream_t s);

// One thread per component: a selected one writes info[id]; first = start (scene) or the label.
hipError_t pieces_emit(const PieceAcc* accs, uint32_t k, uint32_t scene, vxrt_piece* info, hipStream_t s);

// Over the n sorted entries: label[sorted[i]] = the component's label, id[sorted[i]] = its number; either may be null.
hipError_t pieces_scatter(const uint32_t* sorted, const uint32_t* rank, uint32_t n, const uint32_t* comp, const uint32_t* slot,
                          const PieceAcc* accs, uint32_t* label, uint32_t* id, hipStream_t s);

// Over the n input indices: a picked entry's piece number goes to the offset of the picked entries before it.
hipError_t pieces_write(const uint32_t* pick, uint32_t n, const uint64_t* pick_part, const PieceAcc* accs, uint32_t* piece, hipStream_t s);

// ---- api_pieces.hip: the bodies behind the entry points of vxrt_pieces.h and vxrt_components.h -----------------------------------------
// who: the entry point the caller used, which every error text names.
// vxrt_component_table_device as declared; vxrt_label_components_device is this with id = info = nullptr, info_cap = 0.
int component_table(const char* who, vxrt_ctx* c, const int16_t (*pos)[3], size_t n, uint32_t connectivity, uint32_t* label, uint32_t* id,
                    vxrt_piece* info, size_t info_cap, size_t* n_components);

// vxrt_detached_pieces_device as declared (n_pieces not null).  n_pieces == nullptr: vxrt_detached_voxels_device, every detached voxel
// whatever its component's size, with piece = info = nullptr; no accumulators are kept.
int detached_pieces(const char* who, vxrt_ctx* c, const int32_t anchor_min[3], const int32_t anchor_max[3], uint32_t connectivity,
                    uint32_t min_voxels, uint32_t max_voxels, int16_t (*pos)[3], uint8_t (*mrgb)[4], uint32_t* piece, size_t cap, size_t* n,
                    vxrt_piece* info, size_t info_cap, size_t* n_pieces);

}  // namespace vxrt
