// sushi_amd/csrc/track_order_wide_core.hpp -- the host side of the wide ordered tracking pass (include/sushi_hip.h "wide ordered
// tracking"): a call's arguments -> a refusal, or the facts of its launches, and the workspace's layout.  Plain C++,
// host only.  There is no arithmetic here: a wide ordered row is track_wide_core.hpp's wide_near beside track_order_core.hpp's /
// track_order_margin_core.hpp's jump term, each unchanged (tests/host_track_order_wide_check.cpp runs the two together on the CPU).
#ifndef SUSHI_TRACK_ORDER_WIDE_CORE_HPP
#define SUSHI_TRACK_ORDER_WIDE_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "track_order_core.hpp"
#include "track_order_margin_core.hpp"
#include "track_wide_core.hpp"

namespace sushi {

// workspace: the ordered call's layout, then the window records of one row (wide_layout_of)
inline size_t order_wide_layout_bytes(int n_rows, int64_t n_shift) {
    const size_t plain = order_layout_bytes(n_rows, n_shift);
    return plain == 0 ? 0 : wide_layout_of(plain, (int32_t)n_shift).bytes;
}
inline size_t order_margin_wide_layout_bytes(int n_rows, int64_t n_shift) {
    const size_t plain = order_margin_layout_bytes(n_rows, n_shift);
    return plain == 0 ? 0 : wide_layout_of(plain, (int32_t)n_shift).bytes;
}

struct OrderWideStage {
    OrderStage plain;
    WideLayout wide;
    unsigned tile_grid;
    int n_wide;                 // rows of the call that go through the wide kernels
};

// stage_track_ordered's refusals in its order, with stage_track_wide in stage_track's place: the reach's bound is
// TRACK_WIDE_MAX_REACH, and where stage_track looks at a row's reach -- EINVAL for a used reach above TRACK_MAX_REACH beside a
// step_cost that is not +-0.0.  Then the backs and the penalties, EALIGN and ENOSPACE (this layout's bytes), as there.
inline int stage_track_ordered_wide(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* back, const double* penalty,
                                    int n_rows, int32_t n_shift, int64_t n_curve, int method, double step_cost, int row0, int n_total,
                                    const void* mem, size_t mem_bytes, OrderWideStage& out) {
    if (!back || !penalty) return SUSHI_HIP_EINVAL;
    TrackWideStage shared;
    const int rc = stage_track_wide(rows, reach, n_rows, n_shift, n_curve, method, 0.0, step_cost, row0, n_total,
                                    mem ? (const void*)(uintptr_t)256 : nullptr, SIZE_MAX, shared);
    if (rc != SUSHI_HIP_OK) return rc;
    for (int i = 0; i < n_rows; ++i) {
        if (back[i] < TRACK_BACK_ANY) return SUSHI_HIP_EINVAL;
        if ((row0 > 0 || i > 0) && (!isfinite(penalty[i]) || penalty[i] < 0.0)) return SUSHI_HIP_EINVAL;
    }
    out.plain.split = shared.plain.split;
    out.plain.lay = order_layout(n_shift);
    out.wide = wide_layout_of(out.plain.lay.bytes, n_shift);
    out.tile_grid = shared.tile_grid;
    out.n_wide = shared.n_wide;
    if ((uintptr_t)mem & 255) return SUSHI_HIP_EALIGN;
    if (mem_bytes < out.wide.bytes) return SUSHI_HIP_ENOSPACE;
    return SUSHI_HIP_OK;
}

struct OrderMarginWideStage {
    OrderMarginStage plain;
    WideLayout wide;
    unsigned tile_grid;
    int n_wide;
};

// stage_order_margins' refusals in its order, with stage_margins_wide in stage_margins' place: the same two changes.
inline int stage_order_margins_wide(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* back, const double* penalty,
                                    const int32_t* guard, int n_rows, int32_t n_shift, int64_t n_curve, int method, double step_cost,
                                    int row0, int n_total, const void* mem, size_t mem_bytes, OrderMarginWideStage& out) {
    if (!back || !penalty) return SUSHI_HIP_EINVAL;
    MarginWideStage shared;
    const int rc = stage_margins_wide(rows, reach, guard, n_rows, n_shift, n_curve, method, 0.0, step_cost, row0, n_total,
                                      mem ? (const void*)(uintptr_t)256 : nullptr, SIZE_MAX, shared);
    if (rc != SUSHI_HIP_OK) return rc;
    const int used = shared.plain.first_call ? n_rows - 1 : n_rows;       // entries 1 .. used
    for (int i = 1; i <= used; ++i) {
        if (back[i] < TRACK_BACK_ANY) return SUSHI_HIP_EINVAL;
        if (!isfinite(penalty[i]) || penalty[i] < 0.0) return SUSHI_HIP_EINVAL;
    }
    out.plain.split = shared.plain.split;
    out.plain.first_call = shared.plain.first_call;
    out.plain.lay = order_margin_layout(n_shift);
    out.wide = wide_layout_of(out.plain.lay.bytes, n_shift);
    out.tile_grid = shared.tile_grid;
    out.n_wide = shared.n_wide;
    if ((uintptr_t)mem & 255) return SUSHI_HIP_EALIGN;
    if (mem_bytes < out.wide.bytes) return SUSHI_HIP_ENOSPACE;
    return SUSHI_HIP_OK;
}

}  // namespace sushi
#endif
