// sushi_amd/csrc/track_order_core.hpp -- the arithmetic of sushi_hip_track_forward_ordered (include/sushi_hip.h "ordered tracking";
// DESIGN.md 3.21) that track_core.hpp does not already hold: a jump that may go back by at most back_e shifts, at a penalty of its
// row's own.  Plain C++: sushi_track_order.hip runs it on the device, tests/host_track_order_check.cpp on the CPU (g++), both
// compiled with -ffp-contract=off.  The candidates of a move, track_step and the move word are track_core.hpp's, unchanged.  Here:
// the (value, index) combine rule of the prefix minimum and t_e(j); host only, stage_track_ordered -- a call's arguments -> a
// refusal, or the facts of its launches, plain or wide -- and the workspace's layout; host and device, the backtrack's one walker.
#ifndef SUSHI_TRACK_ORDER_CORE_HPP
#define SUSHI_TRACK_ORDER_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "track_core.hpp"

namespace sushi {

constexpr int32_t TRACK_BACK_ANY = SUSHI_HIP_TRACK_BACK_ANY;        // a back: the jump into this row may come from anywhere

// One element of the prefix minimum: P[t] = v, A[t] = i.  No element: (INFINITY, PATH_NO_INDEX).
struct OrderMin { double v; int32_t i; };
SUSHI_GEOM_HD inline OrderMin order_none() { return OrderMin{INFINITY, PATH_NO_INDEX}; }

// (min, first index) of two spans of one row: the smaller value, and of equal values (0.0 and -0.0 are equal) the lower index --
// path_min_replaces, so the result does not depend on the order spans meet in, and with `left` the span of the lower indices it
// is the scan upwards with a strict <.  The value is one of the two operands itself: a zero keeps its sign.
SUSHI_GEOM_HD inline OrderMin order_combine(OrderMin left, OrderMin right) {
    const bool take = path_min_replaces(right.v, right.i, left.v, left.i);
    return OrderMin{take ? right.v : left.v, take ? right.i : left.i};
}

// t_e(j): the last index of row e - 1 a jump into (e, j) may come from; 64 bits, so j + back cannot wrap
SUSHI_GEOM_HD inline int32_t order_reach_back(int64_t j, int32_t back, int32_t n_shift) {
    const int64_t t = j + (int64_t)back;
    return (int32_t)(back < 0 || t > (int64_t)n_shift - 1 ? (int64_t)n_shift - 1 : t);
}

// jump_e[j] = P_{e-1}[t_e(j)] + penalty_e (one rounding); what track_step takes as its `jump`
SUSHI_GEOM_HD inline double order_jump(double p_at_t, double penalty) { return p_at_t + penalty; }

// ---- the host side of a call ----
// The axis is cut as track_split cuts it; a work item is also one tile of the prefix pass.  workspace: one set of path_layout's
// partial records (one per workgroup of the step's grid: the row's minimum and its own extremum), then one record per work item
// -- [min of D over the item: f64][its first index: i32] -- and the same again for what lies before the item (the exclusive scan of
// the first), each array padded to 256 bytes.
struct OrderLayout {
    PathLayout partials;                                // set 0 alone is used
    size_t item_min, item_arg, before_min, before_arg, bytes;
};
inline OrderLayout order_layout(int32_t n_shift) {
    const PathSplit s = track_split(n_shift);
    OrderLayout l;
    l.partials = path_layout_of(s.grid);
    const size_t n = (size_t)s.n_items;
    l.item_min = l.partials.set_bytes;
    l.item_arg = l.item_min + align_up(8 * n, 256);
    l.before_min = l.item_arg + align_up(4 * n, 256);
    l.before_arg = l.before_min + align_up(8 * n, 256);
    l.bytes = l.before_arg + align_up(4 * n, 256);
    return l;
}
inline size_t order_layout_bytes(int n_rows, int64_t n_shift) {
    return n_rows < 1 || n_shift < 1 || n_shift > INT32_MAX ? 0 : order_layout((int32_t)n_shift).bytes;
}

inline size_t order_wide_layout_bytes(int n_rows, int64_t n_shift) {
    const size_t plain = order_layout_bytes(n_rows, n_shift);
    return plain == 0 ? 0 : wide_layout_of(plain, (int32_t)n_shift).bytes;
}

struct OrderStage : TrackCall {
    OrderLayout lay;
};

// EINVAL: a null back or penalty table; track_rows_check's (there is no one penalty to check: it is made per row here); a back
// below TRACK_BACK_ANY; a penalty that is not finite or is negative in any row but the sequence's row 0 (whose penalty is ignored,
// as its back is: no jump enters it).  Then track_workspace_check's refusals.  `out` is unspecified after a refusal.
inline int stage_track_ordered(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* back, const double* penalty, int n_rows,
                               int32_t n_shift, int64_t n_curve, int method, double step_cost, int row0, int n_total, const void* mem,
                               size_t mem_bytes, OrderStage& out, bool wide = false) {
    if (!back || !penalty) return SUSHI_HIP_EINVAL;
    const int rc = track_rows_check(rows, reach, mem, n_rows, n_shift, n_curve, method, 0.0, step_cost, row0, n_total, wide, out.n_wide);
    if (rc != SUSHI_HIP_OK) return rc;
    for (int i = 0; i < n_rows; ++i) {
        if (back[i] < TRACK_BACK_ANY) return SUSHI_HIP_EINVAL;
        if ((row0 > 0 || i > 0) && (!isfinite(penalty[i]) || penalty[i] < 0.0)) return SUSHI_HIP_EINVAL;
    }
    out.lay = order_layout(n_shift);
    return track_workspace_check(mem, mem_bytes, out.lay.bytes, n_shift, wide, out);
}

// ---- the backtrack: one walker, on the device (one lane) and on the CPU ----
// s_{E-1} = a_{E-1}; s_{e-1} = move_e[s_e] == TRACK_JUMP ? A_{e-1}[t_e(s_e)] : s_e + move_e[s_e], clamped into the axis
// (from: [n_total][n_shift], row e holds A_e; back: [n_total])
SUSHI_GEOM_HD inline void order_backtrack(const int16_t* move, const int32_t* from, const int32_t* back, const int32_t* row_arg, int n_total,
                                          int32_t n_shift, int32_t* out_shift) {
    int32_t s = path_clamp(row_arg[n_total - 1], n_shift);
    out_shift[n_total - 1] = s;
    for (int e = n_total - 1; e >= 1; --e) {
        const int16_t m = move[(int64_t)e * n_shift + s];
        const int64_t to = (int64_t)s + m;
        const int32_t b = back[e] < TRACK_BACK_ANY ? TRACK_BACK_ANY : back[e];
        s = m == TRACK_JUMP ? path_clamp(from[(int64_t)(e - 1) * n_shift + order_reach_back(s, b, n_shift)], n_shift)
                            : (int32_t)(to < 0 ? 0 : (to >= n_shift ? n_shift - 1 : to));
        out_shift[e - 1] = s;
    }
}

}  // namespace sushi
#endif
