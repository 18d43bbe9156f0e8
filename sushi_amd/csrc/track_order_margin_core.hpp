// sushi_amd/csrc/track_order_margin_core.hpp -- the arithmetic of sushi_hip_track_order_margins (include/sushi_hip.h "ordered
// margins") that track_margin_core.hpp and track_order_core.hpp do not already hold: the backward recurrence's jump
// term, a suffix minimum read with the bound on the other side.  Plain C++: sushi_track_order.hip runs it on the device,
// tests/host_track_order_margins_check.cpp on the CPU (g++), both compiled with -ffp-contract=off.  The window minimum, margin_back
// / margin_through / margin_suffix / margin_outside / margin_alt_index and order_combine are theirs, unchanged.  Here: t'_e(j), the
// jump sum and the suffix minimum's combine rule on values alone; host only, the workspace's layout and stage_order_margins -- a
// call's arguments -> a refusal, or the facts of its launches, plain or wide.
#ifndef SUSHI_TRACK_ORDER_MARGIN_CORE_HPP
#define SUSHI_TRACK_ORDER_MARGIN_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "track_margin_core.hpp"
#include "track_order_core.hpp"

namespace sushi {

// t'_e(j): the first index of row e + 1 a jump out of (e, j) may go to, max(j - back_{e+1}, 0); 64 bits, so j - back cannot wrap
SUSHI_GEOM_HD inline int32_t order_margin_from(int64_t j, int32_t back) {
    const int64_t t = j - (int64_t)back;
    return (int32_t)(back < 0 || t < 0 ? 0 : t);
}

// jumpB[j] = S_{e+1}[t'_e(j)] + penalty_{e+1} (one rounding); what margin_back takes as its `jump`
SUSHI_GEOM_HD inline double order_margin_jump(double s_at_t, double penalty) { return s_at_t + penalty; }

// The suffix minimum of two adjacent spans of one row, `lo` the span of the lower indices: the smaller value, and of equal values
// (0.0 and -0.0 are equal) the lower span's -- the value of order_combine with the spans' first indices, which two adjacent spans
// need not carry: the leftmost of the smallest values does not depend on the grouping.  The value is one of the two operands
// itself: a zero keeps its sign.
SUSHI_GEOM_HD inline double order_suffix_combine(double lo, double hi) { return lo <= hi ? lo : hi; }

// ---- the host side of a call ----
// The axis is cut as track_split cuts it; a work item is also one tile of the suffix pass.  workspace: one set of margin_layout's
// partial records (three first minima per workgroup of the step's grid; the scan of the same row reads them, so one set is
// enough), then one record per work item -- [min of C over the item: f64][its first index: i32] -- and [f64] the minimum of
// everything after the item (the exclusive suffix scan of the first), each array padded to 256 bytes.
struct OrderMarginLayout {
    MarginLayout partials;                              // set 0 alone is used
    size_t item_min, item_arg, after_min, bytes;
};
inline OrderMarginLayout order_margin_layout(int32_t n_shift) {
    const PathSplit s = track_split(n_shift);
    OrderMarginLayout l;
    l.partials = margin_layout_of(s.grid);
    const size_t n = (size_t)s.n_items;
    l.item_min = l.partials.set_bytes;
    l.item_arg = l.item_min + align_up(8 * n, 256);
    l.after_min = l.item_arg + align_up(4 * n, 256);
    l.bytes = l.after_min + align_up(8 * n, 256);
    return l;
}
inline size_t order_margin_layout_bytes(int n_rows, int64_t n_shift) {
    return n_rows < 1 || n_shift < 1 || n_shift > INT32_MAX ? 0 : order_margin_layout((int32_t)n_shift).bytes;
}

inline size_t order_margin_wide_layout_bytes(int n_rows, int64_t n_shift) {
    const size_t plain = order_margin_layout_bytes(n_rows, n_shift);
    return plain == 0 ? 0 : wide_layout_of(plain, (int32_t)n_shift).bytes;
}

struct OrderMarginStage : TrackCall {
    OrderMarginLayout lay;
    bool first_call;            // row0 + n_rows == n_total: the call begins at the sequence's last row
};

// The tables are stage_margins': rows[i] and guard[i] are row row0 + i's; reach[i], back[i] and penalty[i] are row row0 + i's for
// i = 0 .. n_rows, the last only where that row exists; entry 0 is not used and is ignored.  EINVAL: a null back or penalty table;
// margin_rows_check's (there is no one penalty to check); a used back below TRACK_BACK_ANY; a used penalty that is not finite or is
// negative.  Then track_workspace_check's refusals.  `out` is unspecified after a refusal.
inline int stage_order_margins(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* back, const double* penalty,
                               const int32_t* guard, int n_rows, int32_t n_shift, int64_t n_curve, int method, double step_cost, int row0,
                               int n_total, const void* mem, size_t mem_bytes, OrderMarginStage& out, bool wide = false) {
    if (!back || !penalty) return SUSHI_HIP_EINVAL;
    const int rc = margin_rows_check(rows, reach, guard, mem, n_rows, n_shift, n_curve, method, 0.0, step_cost, row0, n_total, wide,
                                     out.first_call, out.n_wide);
    if (rc != SUSHI_HIP_OK) return rc;
    const int used = out.first_call ? n_rows - 1 : n_rows;          // entries 1 .. used
    for (int i = 1; i <= used; ++i) {
        if (back[i] < TRACK_BACK_ANY) return SUSHI_HIP_EINVAL;
        if (!isfinite(penalty[i]) || penalty[i] < 0.0) return SUSHI_HIP_EINVAL;
    }
    out.lay = order_margin_layout(n_shift);
    return track_workspace_check(mem, mem_bytes, out.lay.bytes, n_shift, wide, out);
}

// back_{e+1} and penalty_{e+1} for the launch of row row0 + i: no limit and 0 for the sequence's last row, which has no row after
// it (neither is used there)
inline int32_t order_margin_back_after(const int32_t* back, int i, int n_rows, bool first_call) {
    return i == n_rows - 1 && first_call ? TRACK_BACK_ANY : back[i + 1];
}
inline double order_margin_penalty_after(const double* penalty, int i, int n_rows, bool first_call) {
    return i == n_rows - 1 && first_call ? 0.0 : penalty[i + 1];
}

}  // namespace sushi
#endif
