// sushi_amd/csrc/track_order_wide_core.hpp -- the host side of the wide ordered tracking pass (include/sushi_hip.h "wide ordered
// tracking") in one include: track_order_core.hpp's and track_order_margin_core.hpp's stages and layouts,
// track_wide_core.hpp's wide_near, and the two stages with `wide` set by names of their own.  Plain C++, host only.  There is no
// arithmetic and no checking body here: a wide ordered row is wide_near beside the ordered pass's jump term, each unchanged
// (tests/host_track_order_wide_check.cpp runs the two together on the CPU), and the refusals are stage_track_ordered's and
// stage_order_margins'.
#ifndef SUSHI_TRACK_ORDER_WIDE_CORE_HPP
#define SUSHI_TRACK_ORDER_WIDE_CORE_HPP

#include "track_order_core.hpp"
#include "track_order_margin_core.hpp"
#include "track_wide_core.hpp"

namespace sushi {

using OrderWideStage = WideStageOf<OrderStage>;
using OrderMarginWideStage = WideStageOf<OrderMarginStage>;

inline int stage_track_ordered_wide(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* back, const double* penalty,
                                    int n_rows, int32_t n_shift, int64_t n_curve, int method, double step_cost, int row0, int n_total,
                                    const void* mem, size_t mem_bytes, OrderWideStage& out) {
    const int rc = stage_track_ordered(rows, reach, back, penalty, n_rows, n_shift, n_curve, method, step_cost, row0, n_total, mem,
                                       mem_bytes, out.plain, true);
    static_cast<TrackCall&>(out) = out.plain;
    return rc;
}
inline int stage_order_margins_wide(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* back, const double* penalty,
                                    const int32_t* guard, int n_rows, int32_t n_shift, int64_t n_curve, int method, double step_cost,
                                    int row0, int n_total, const void* mem, size_t mem_bytes, OrderMarginWideStage& out) {
    const int rc = stage_order_margins(rows, reach, back, penalty, guard, n_rows, n_shift, n_curve, method, step_cost, row0, n_total, mem,
                                       mem_bytes, out.plain, true);
    static_cast<TrackCall&>(out) = out.plain;
    return rc;
}

}  // namespace sushi
#endif
