// setops_rule.h — the arithmetic of include/vxrt_setops.h as the kernel runs it (setops.hip) and as a host compiler reads it
// (tests/test_setops_cpu.py builds a program of its own around this file): the co-rank of a diagonal of the merge of two ascending
// unique key arrays, the two membership tests and the ops' keep rule.  Nothing from HIP is included, and the marker below is empty
// for a compiler that is not hipcc.  DESIGN.md §24.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VXRT_SETOPS_FN __host__ __device__ inline
#else
#define VXRT_SETOPS_FN inline
#endif

namespace vxrt {

// vxrt_list_op
constexpr uint32_t kListUnion = 0, kListIntersect = 1, kListDifference = 2, kListXor = 3, kListChanged = 4;

// The tile of a block and the run of a thread: kSetopSpan consecutive items of the merged sequence per block, kSetopItems per thread.
constexpr uint32_t kSetopThreads = 256;
constexpr uint32_t kSetopItems = 8;
constexpr uint32_t kSetopSpan = kSetopThreads * kSetopItems;
// What stands where A[-1] and B[nb] would: no key (48 bits) equals it.
constexpr uint64_t kSetopNoKey = ~uint64_t(0);

// The merged sequence of a[0 .. na) and b[0 .. nb) (each ascending and unique, na + nb < 2^32) has na + nb items; on equal keys a's
// item comes first.  Of its first `diag` items (diag <= na + nb) merge_corank are a's, and diag - merge_corank are b's: the least i
// of [max(0, diag - nb), min(diag, na)] with  i == min(diag, na)  or  a[i] > b[diag - 1 - i]  ("a[i] <= b[j - 1]" puts a[i] in front
// of b[j - 1], so a prefix that holds b[j - 1] holds a[i] too).  That test is true and then false along the diagonal, so the least i
// is found by halving; every index read lies in [0, na) or [0, nb).  The range has at most 2^32 - 1 values: 32 steps at most.
VXRT_SETOPS_FN uint32_t merge_corank(const uint64_t* a, uint32_t na, const uint64_t* b, uint32_t nb, uint32_t diag) {
    uint32_t lo = diag > nb ? diag - nb : 0u, hi = diag < na ? diag : na;
    for (uint32_t step = 0; step < 32u && lo < hi; step++) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= b[diag - 1u - mid]) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// The item the merge takes next at the cursors (i, j): a's when a has one and b has none or a[i] <= b[j].  a_key / b_key are read
// only where the cursor is inside its array (the caller may pass anything else there).
VXRT_SETOPS_FN bool merge_takes_a(bool a_left, uint64_t a_key, bool b_left, uint64_t b_key) {
    return a_left && (!b_left || a_key <= b_key);
}

// Is a's item a[i], taken at b's cursor j, in b?  Every b[< j] is smaller (it came first, and ties go to a) and b[j] is not, so
// exactly when b has a b[j] and it is equal.  b_at_cursor is b[j], or kSetopNoKey when j == nb.
VXRT_SETOPS_FN bool a_item_matched(uint64_t a_key, uint64_t b_at_cursor) { return b_at_cursor == a_key; }

// Is b's item b[j], taken at a's cursor i, in a?  a[i - 1] <= b[j] < a[i], so exactly when there is an a[i - 1] and it is equal.
// a_before_cursor is a[i - 1], or kSetopNoKey when i == 0.  Neither test looks at "the previous merged item", so a pair that lies
// across two threads or two blocks is seen from both sides.
VXRT_SETOPS_FN bool b_item_matched(uint64_t b_key, uint64_t a_before_cursor) { return a_before_cursor == b_key; }

// Is the item part of the result?  A kept item carries the bytes of its own side: UNION drops a's item of a pair and keeps b's
// (last wins), INTERSECT and DIFFERENCE keep only a's items, CHANGED only b's.  words_equal matters for a matched b item of CHANGED.
VXRT_SETOPS_FN bool keep(uint32_t op, bool from_b, bool matched, bool words_equal) {
    return op == kListUnion        ? (from_b || !matched)
           : op == kListIntersect  ? (!from_b && matched)
           : op == kListDifference ? (!from_b && !matched)
           : op == kListXor        ? !matched
                                   : (from_b && !(matched && words_equal));
}

// A load from a "safe index": at where the array has it, else its last entry (entry 0 of an empty array's allocation, which is
// readable), for loads that are issued whether or not their value is used.
VXRT_SETOPS_FN uint32_t safe_index(uint32_t at, uint32_t count) {
    const uint32_t last = count ? count - 1u : 0u;
    return at < last ? at : last;
}

// The index in a of the item in front of a's cursor when b's item b[b_at] is taken as merged item merged_at (both counted over the
// whole lists): the merged position less b's index is a's cursor.  Wraps at cursor 0, where there is no such item: safe_index
// brings it back, and b_item_matched has already said no.
VXRT_SETOPS_FN uint32_t a_index_before(uint32_t merged_at, uint32_t b_at) { return merged_at - b_at - 1u; }

// One thread's run: the items [diag, diag + count) of the merge of a tile's a[0 .. na) and b[0 .. nb), count <= kSetopItems, from the
// cursors the co-rank of diag gives.  a[-1] and b[nb] must be readable: the keys before and behind the tile, or kSetopNoKey where the
// whole list has none.  (a[na] may be read too and is not used.)  Per item k: key[k]; bit k of *from_b and *matched; own[k] = the
// item's index in its own tile array.  Returns the bits of the items that exist.  The loop is kSetopItems steps long.
VXRT_SETOPS_FN uint32_t merge_run(const uint64_t* a, uint32_t na, const uint64_t* b, uint32_t nb, uint32_t diag, uint32_t count, uint64_t* key,
                                  uint32_t* own, uint32_t* from_b, uint32_t* matched) {
    uint32_t i = merge_corank(a, na, b, nb, diag), j = diag - i;
    uint64_t before = a[int32_t(i) - 1], ka = a[i], kb = b[j];
    uint32_t live = 0, fb = 0, hit = 0;
    for (uint32_t k = 0; k < kSetopItems; k++) {
        const bool here = k < count;
        const bool take_a = merge_takes_a(i < na, ka, j < nb, kb);
        const bool m = take_a ? a_item_matched(ka, kb) : b_item_matched(kb, before);     // kb is kSetopNoKey or a later key at j == nb
        key[k] = take_a ? ka : kb;
        own[k] = take_a ? i : j;
        live |= (here ? 1u : 0u) << k;
        fb |= (here && !take_a ? 1u : 0u) << k;
        hit |= (here && m ? 1u : 0u) << k;
        if (here && take_a) {
            before = ka;
            i++;
            ka = a[i];
        } else if (here && j < nb) {      // always, when count is within the tile; the test keeps j <= nb whatever the caller passes
            j++;
            kb = b[j];
        }
    }
    *from_b = fb;
    *matched = hit;
    return live;
}

}  // namespace vxrt
