// sushi_amd/csrc/path_core.hpp -- the arithmetic of sushi_hip_path_forward (include/sushi_hip.h "segmentation"),
// one shift index at a time.  Plain C++: sushi_path.hip runs it on the device, tests/host_path_check.cpp on the CPU (g++).  Both are
// compiled with -ffp-contract=off: the product of a weighted cost and the sum of a step round separately, as NumPy's do.
// Behind it, host only: the workspace's layout, and stage_path -- a call's arguments -> a refusal, or the facts of its launches.
#ifndef SUSHI_PATH_CORE_HPP
#define SUSHI_PATH_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "axis_core.hpp"           // the first-extremum rule, the row check, the work split

namespace sushi {

// u_e[j]: the weighted cost of one score.  The cost of a value is the value itself where the smaller score is the better one
// (SQDIFF_NORMED) and its exact negation where the larger one is (CCOEFF_NORMED); the product rounds once.
SUSHI_GEOM_HD inline double path_cost(int method, double w, float v) {
    const double c = method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? -(double)v : (double)v;
    return w * c;
}

// D_e[j] from D_{e-1}[j], u_e[j] and jump_e = m_{e-1} + penalty.  *stay: the path into (e, j) comes from (e - 1, j); a tie stays.
SUSHI_GEOM_HD inline double path_step(double d_prev, double u, double jump, bool* stay) {
    *stay = d_prev <= jump;
    return u + (*stay ? d_prev : jump);
}

// Whether (v, i) replaces (best, at) as the first minimum, in whatever order the candidates meet: the smaller value, and of equal
// values (0.0 and -0.0 are equal) the lower index.  No element: at = PATH_NO_INDEX, which every real index beats on a tie.
constexpr int32_t PATH_NO_INDEX = INT32_MAX;
// (| and &, not || and &&: the device code takes no branch for it)
SUSHI_GEOM_HD inline bool path_min_replaces(double v, int32_t i, double best, int32_t at) {
    return ((int)(v < best) | ((int)(v == best) & (int)(i < at))) != 0;
}

// The same for a row's own first extremum (axis_better's rule: strict, so equal values leave the lower index).
SUSHI_GEOM_HD inline bool path_own_replaces(int method, float v, int32_t i, float best, int32_t at) {
    return ((int)axis_better(method, v, best) | ((int)!axis_better(method, best, v) & (int)(i < at))) != 0;
}

// an index a NaN let through (unspecified results) is brought back into the axis: no access leaves the buffers
SUSHI_GEOM_HD inline int32_t path_clamp(int32_t i, int32_t n_shift) { return i < 0 ? 0 : (i >= n_shift ? n_shift - 1 : i); }

// ---- the host side of a call ----
// The shift axis is cut into work items (axis_core.hpp: a wave's 64 consecutive indices are also one whole word of stay bits), of
// AXIS_PER_LARGE where there are at least PATH_FILL such items (four workgroups for each of 256 CUs: n_shift >= 2,095,105).  Every
// workgroup of the grid leaves one partial record.
constexpr int64_t PATH_FILL = 1024;
constexpr int PATH_THREADS = AXIS_THREADS;      // a step kernel's workgroup: the threads of one work item

SUSHI_GEOM_HD inline int64_t path_stay_words(int64_t n_shift) { return n_shift < 1 || n_shift > INT32_MAX ? 0 : (n_shift + 63) / 64; }

struct PathSplit {
    int per;
    int64_t n_items;
    unsigned grid;
};
inline PathSplit path_split(int32_t n_shift) {
    PathSplit s;
    s.per = axis_per(axis_items(n_shift, AXIS_PER_LARGE), PATH_FILL);
    s.n_items = axis_items(n_shift, s.per);
    s.grid = axis_grid(s.n_items);
    return s;
}

// workspace: two sets of partial records, used by turns, each as four arrays of `grid` entries -- [min of D: f64][its index: i32]
// [own extremum's index: i32][own extremum: f32] -- and each set padded to 256 bytes.  Nothing is uploaded: a row's curve_off and
// weight travel as arguments of its launch.
struct PathLayout {
    size_t set_bytes, d_min, d_arg, own_idx, own_val, bytes;    // offsets inside a set; set s starts at s * set_bytes
};
inline PathLayout path_layout_of(size_t g) {        // g: the workgroups of the grid
    PathLayout l;
    l.d_min = 0;
    l.d_arg = l.d_min + 8 * g;
    l.own_idx = l.d_arg + 4 * g;
    l.own_val = l.own_idx + 4 * g;
    l.set_bytes = align_up(l.own_val + 4 * g, 256);
    l.bytes = 2 * l.set_bytes;
    return l;
}
inline PathLayout path_layout(int32_t n_shift) { return path_layout_of(path_split(n_shift).grid); }
inline size_t path_layout_bytes(int n_rows, int64_t n_shift) {
    return n_rows < 1 || n_shift < 1 || n_shift > INT32_MAX ? 0 : path_layout((int32_t)n_shift).bytes;
}

struct PathStage {
    PathSplit split;
    PathLayout lay;
    int64_t words;              // 64-bit words of one row's stay bits
};

// EINVAL: a null table; an unknown method; n_rows < 1, n_shift < 1, n_curve < 1, n_shift > n_curve; row0 < 0, n_total < 1 or rows
// row0 .. row0 + n_rows - 1 not inside [0, n_total) (decided without forming a sum that could pass int); a row that leaves the curve
// buffer (curve_off < 0 or curve_off > n_curve - n_shift: no sum is formed); a weight or a penalty that is not finite or is
// negative.  Then EALIGN: a workspace that is not 256-byte aligned; ENOSPACE: mem_bytes below the layout's.  `out` is unspecified
// after a refusal.
inline int stage_path(const SushiHipJointRow* rows, int n_rows, int32_t n_shift, int64_t n_curve, int method, double penalty,
                      int row0, int n_total, const void* mem, size_t mem_bytes, PathStage& out) {
    if (!rows || !mem) return SUSHI_HIP_EINVAL;
    if (!method_known(method)) return SUSHI_HIP_EINVAL;
    if (n_rows < 1 || n_shift < 1 || n_curve < 1 || n_shift > n_curve) return SUSHI_HIP_EINVAL;
    if (n_total < 1 || row0 < 0 || row0 >= n_total || n_rows > n_total - row0) return SUSHI_HIP_EINVAL;
    if (!isfinite(penalty) || penalty < 0.0) return SUSHI_HIP_EINVAL;
    for (int i = 0; i < n_rows; ++i)
        if (!axis_row_ok(rows[i], n_curve, n_shift)) return SUSHI_HIP_EINVAL;
    out.split = path_split(n_shift);
    out.lay = path_layout(n_shift);
    out.words = path_stay_words(n_shift);
    if ((uintptr_t)mem & 255) return SUSHI_HIP_EALIGN;
    if (mem_bytes < out.lay.bytes) return SUSHI_HIP_ENOSPACE;
    return SUSHI_HIP_OK;
}

// ---- the backtrack: one walker, on the device (one lane) and on the CPU ----
// s_{E-1} = a_{E-1}; s_{e-1} = stay_e[s_e] ? s_e : a_{e-1}
SUSHI_GEOM_HD inline void path_backtrack(const uint64_t* stay, const int32_t* row_arg, int n_total, int32_t n_shift, int32_t* out_shift) {
    const int64_t words = path_stay_words(n_shift);
    int32_t s = path_clamp(row_arg[n_total - 1], n_shift);
    out_shift[n_total - 1] = s;
    for (int e = n_total - 1; e >= 1; --e) {
        if (!((stay[(int64_t)e * words + (s >> 6)] >> (s & 63)) & 1)) s = path_clamp(row_arg[e - 1], n_shift);
        out_shift[e - 1] = s;
    }
}

}  // namespace sushi
#endif
