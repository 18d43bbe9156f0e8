// sushi_amd/csrc/track_margin_core.hpp -- the arithmetic of sushi_hip_track_margins (include/sushi_hip.h "margins"),
// one shift index at a time, on top of track_core.hpp's candidates.  Plain C++: sushi_track.hip runs it on the device,
// tests/host_track_margins_check.cpp on the CPU (g++).  Both are compiled with -ffp-contract=off.  Behind it, host only: the
// workspace's layout (three first minima per workgroup) and stage_margins -- a call's arguments -> a refusal, or the facts of its
// launches, plain or wide.
#ifndef SUSHI_TRACK_MARGIN_CORE_HPP
#define SUSHI_TRACK_MARGIN_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "track_core.hpp"

namespace sushi {

// B_e[j] from nearB[j] (track_price / track_cand over C_{e+1}, the value only) and jumpB = n_{e+1} + penalty: a tie moves, as in
// track_step.
SUSHI_GEOM_HD inline double margin_back(double near, double jump) { return near <= jump ? near : jump; }
// M_e[j] = D_e[j] + B_e[j] and C_e[j] = u_e[j] + B_e[j] (track_step's operand order): one rounding each.  The sequence's last row
// has no B: M is D itself and C is u itself (nothing is added: the bits of D).
SUSHI_GEOM_HD inline double margin_through(double d, double b, bool last) { return last ? d : d + b; }
SUSHI_GEOM_HD inline double margin_suffix(double u, double b, bool last) { return last ? u : u + b; }
// whether index j lies more than `guard` samples from s (64 bits: a guard up to INT32_MAX forms no sum that overflows)
SUSHI_GEOM_HD inline bool margin_outside(int64_t j, int32_t s, int32_t guard) {
    return ((int)(j < (int64_t)s - guard) | (int)(j > (int64_t)s + guard)) != 0;
}
// an alternative's index as it is stored: -1 where no index lies outside the guard window
constexpr int32_t MARGIN_NO_ALT = -1;
SUSHI_GEOM_HD inline int32_t margin_alt_index(int32_t i, int32_t n_shift) { return i == PATH_NO_INDEX ? MARGIN_NO_ALT : path_clamp(i, n_shift); }

// ---- the host side of a call ----
// The axis is cut as the tracking pass cuts it (track_split: the same tile of PER * 256 values and a halo of the reach on each
// side).  workspace: two sets of partial records, used by turns, each as six arrays of `grid` entries -- the first minimum of C, of M
// and of M outside the guard window: [f64][f64][f64][i32][i32][i32] -- and each set padded to 256 bytes.
struct MarginLayout {
    size_t set_bytes, c_min, m_min, a_min, c_arg, m_arg, a_arg, bytes;      // offsets inside a set; set s starts at s * set_bytes
};
inline MarginLayout margin_layout_of(size_t g) {
    MarginLayout l;
    l.c_min = 0;
    l.m_min = 8 * g;
    l.a_min = 16 * g;
    l.c_arg = 24 * g;
    l.m_arg = 28 * g;
    l.a_arg = 32 * g;
    l.set_bytes = align_up(36 * g, 256);
    l.bytes = 2 * l.set_bytes;
    return l;
}
inline MarginLayout margin_layout(int32_t n_shift) { return margin_layout_of(track_split(n_shift).grid); }
inline size_t margin_layout_bytes(int n_rows, int64_t n_shift) {
    return n_rows < 1 || n_shift < 1 || n_shift > INT32_MAX ? 0 : margin_layout((int32_t)n_shift).bytes;
}

inline size_t margin_wide_layout_bytes(int n_rows, int64_t n_shift) {
    const size_t plain = margin_layout_bytes(n_rows, n_shift);
    return plain == 0 ? 0 : wide_layout_of(plain, (int32_t)n_shift).bytes;
}

struct MarginStage : TrackCall {
    MarginLayout lay;
    bool first_call;            // row0 + n_rows == n_total: the call begins at the sequence's last row
};

// The call walks rows row0 + n_rows - 1 down to row0 of a sequence of n_total rows.  rows[i] and guard[i] are row row0 + i's;
// reach[i] is row row0 + i's for i = 0 .. n_rows, the last only where that row exists (row0 + n_rows < n_total); reach[0] is not
// used (the step into row row0 is priced when the row before it is walked) and is ignored.
// The margins walks' EINVALs: a null guard table and track_args_check's; a row that leaves the curve buffer or a weight that is
// not finite or is negative; a used reach that is not track_reach_ok; a guard < 0.
inline int margin_rows_check(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* guard, const void* mem, int n_rows,
                             int32_t n_shift, int64_t n_curve, int method, double penalty, double step_cost, int row0, int n_total,
                             bool wide, bool& first_call, int& n_wide) {
    if (!guard) return SUSHI_HIP_EINVAL;
    const int rc = track_args_check(rows, reach, mem, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total);
    if (rc != SUSHI_HIP_OK) return rc;
    first_call = n_rows == n_total - row0;
    n_wide = 0;
    const int used_to = first_call ? n_rows - 1 : n_rows;                  // reach[1 .. used_to] are used
    for (int i = 0; i <= used_to; ++i) {
        if (i < n_rows && !axis_row_ok(rows[i], n_curve, n_shift)) return SUSHI_HIP_EINVAL;
        if (i > 0 && !track_reach_ok(reach[i], step_cost, wide, n_wide)) return SUSHI_HIP_EINVAL;
        if (i < n_rows && guard[i] < 0) return SUSHI_HIP_EINVAL;
    }
    return SUSHI_HIP_OK;
}

// margin_rows_check's refusals, then track_workspace_check's.  `out` is unspecified after a refusal.
inline int stage_margins(const SushiHipJointRow* rows, const int32_t* reach, const int32_t* guard, int n_rows, int32_t n_shift,
                         int64_t n_curve, int method, double penalty, double step_cost, int row0, int n_total, const void* mem,
                         size_t mem_bytes, MarginStage& out, bool wide = false) {
    const int rc = margin_rows_check(rows, reach, guard, mem, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total, wide,
                                     out.first_call, out.n_wide);
    if (rc != SUSHI_HIP_OK) return rc;
    out.lay = margin_layout(n_shift);
    return track_workspace_check(mem, mem_bytes, out.lay.bytes, n_shift, wide, out);
}

// reach_{e+1} for the launch of row row0 + i: 0 for the sequence's last row, which has no row after it
inline int32_t margin_reach_after(const int32_t* reach, int i, int n_rows, bool first_call) {
    return i == n_rows - 1 && first_call ? 0 : reach[i + 1];
}

}  // namespace sushi
#endif
