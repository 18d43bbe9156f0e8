// sushi_amd/csrc/axis_core.hpp -- what the calls that lay score rows (sushi_hip_match_curves output) on one shift axis share: the
// joint search (joint_core.hpp) and the segmentation pass (path_core.hpp).  The first-extremum rule,
// the check of a row, how an axis is cut into work items, and the index a load past the axis's end is moved onto.  Plain C++, host
// and device; included by those two headers only.
#ifndef SUSHI_AXIS_CORE_HPP
#define SUSHI_AXIS_CORE_HPP

#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/sushi_hip.h"
#include "sushi_geometry.hpp"      // SUSHI_GEOM_HD, method_known, align_up

namespace sushi {

// Whether `v` replaces `best` as the extremum when the values are visited in ascending index order: the FIRST minimum
// (SQDIFF_NORMED) or maximum (CCOEFF_NORMED) wins; 0.0 and -0.0 tie.
SUSHI_GEOM_HD inline bool axis_better(int method, float v, float best) {
    return method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? v > best : v < best;
}

// A row of n_shift scores stays inside a curve buffer of n_curve floats (curve_off + n_shift <= n_curve, without forming the sum),
// and its weight is finite and not negative.
inline bool axis_row_ok(const SushiHipJointRow& r, int64_t n_curve, int64_t n_shift) {
    return r.curve_off >= 0 && r.curve_off <= n_curve - n_shift && isfinite(r.weight) && r.weight >= 0.0;
}

// An axis is cut into work items of PER * AXIS_THREADS consecutive indices, one workgroup each; thread t of an item holds the
// indices t, t + AXIS_THREADS, ...: a wave's 64 lanes hold 64 consecutive indices from a multiple of 64 on, so its load of one row
// is one contiguous span wherever the row starts.  PER is AXIS_PER_LARGE where there are enough such items to fill the GPU (a
// threshold of the caller's), else AXIS_PER_SMALL (a quarter of the indices each, four times the items).  A grid of at most
// AXIS_MAX_GRID workgroups (256 CUs, eight each) strides over the items.
constexpr int AXIS_THREADS = 256;
constexpr int AXIS_PER_LARGE = 8, AXIS_PER_SMALL = 2;
constexpr int64_t AXIS_MAX_GRID = 2048;

inline int64_t axis_items(int64_t n_shift, int per) { return (n_shift + per * AXIS_THREADS - 1) / (per * AXIS_THREADS); }
inline int axis_per(int64_t items_large, int64_t fill) { return items_large >= fill ? AXIS_PER_LARGE : AXIS_PER_SMALL; }
inline unsigned axis_grid(int64_t n_items) { return (unsigned)(n_items < AXIS_MAX_GRID ? n_items : AXIS_MAX_GRID); }

// Where a thread's load of index j goes: the indices past the axis's end are moved onto its last one.  A load that is always made
// needs no branch, and the loads of several rows can be counted in flight; what such a load returns is not used.
SUSHI_GEOM_HD inline int32_t axis_at(int64_t j, int32_t n_shift) { return (int32_t)(j < n_shift ? j : n_shift - 1); }

// A kernel instantiated per <PER, MAX>: `f` launches it with the template arguments it is given, as integral constants.
template <typename F> void axis_dispatch(int per, bool max, F&& f) {
    if (per == AXIS_PER_LARGE) {
        if (max) f(std::integral_constant<int, AXIS_PER_LARGE>(), std::true_type());
        else f(std::integral_constant<int, AXIS_PER_LARGE>(), std::false_type());
    } else {
        if (max) f(std::integral_constant<int, AXIS_PER_SMALL>(), std::true_type());
        else f(std::integral_constant<int, AXIS_PER_SMALL>(), std::false_type());
    }
}

}  // namespace sushi
#endif
