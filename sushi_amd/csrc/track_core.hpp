// sushi_amd/csrc/track_core.hpp -- the arithmetic of sushi_hip_track_forward (include/sushi_hip.h "tracking"), one
// candidate at a time.  Plain C++: sushi_track.hip runs it on the device, tests/host_track_check.cpp on the CPU (g++).  Both are
// compiled with -ffp-contract=off: the price of a move (a product) and the candidate it is added to round separately, as NumPy's do.
// Behind it, host only: what the four walks' stages share and stage_track -- a call's arguments -> a refusal, or the facts of its
// launches, plain or wide -- and, host and device, the backtrack's one walker.  The costs, the first-extremum rules, the partial
// records and their workspace are path_core.hpp's.
#ifndef SUSHI_TRACK_CORE_HPP
#define SUSHI_TRACK_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "path_core.hpp"

namespace sushi {

constexpr int32_t TRACK_MAX_REACH = SUSHI_HIP_TRACK_MAX_REACH;      // the most samples the shift may move between two events
constexpr int16_t TRACK_JUMP = SUSHI_HIP_TRACK_JUMP;                // a move word: the path into (e, j) comes from a_{e-1}

// cand(d) for d != 0: D_{e-1}[j + d] + step_cost * |d|.  The product rounds once, then the sum rounds once.  (cand(0) is
// D_{e-1}[j] itself: nothing is added, so -0.0 keeps its bits.)
SUSHI_GEOM_HD inline double track_price(double step_cost, int32_t a) { return step_cost * (double)a; }
SUSHI_GEOM_HD inline double track_cand(double d_prev, double price) { return d_prev + price; }

// Whether the candidate (v, d) replaces (best, bd) as near_e[j], in whatever order the candidates meet: the smaller value; of equal
// values (0.0 and -0.0 are equal) the smaller |d|; of those the negative d.  A total order on (value, |d|, d > 0).
// (| and &, not || and &&: the device code takes no branch for it)
SUSHI_GEOM_HD inline bool track_replaces(double v, int32_t d, double best, int32_t bd) {
    const int32_t ad = d < 0 ? -d : d, abd = bd < 0 ? -bd : bd;
    return ((int)(v < best) | ((int)(v == best) & ((int)(ad < abd) | ((int)(ad == abd) & (int)(d < bd))))) != 0;
}

// The same rule where the candidates are visited in the order 0, -1, +1, -2, +2, ...: a later candidate never wins a tie, so the
// strict comparison alone decides (the kernel's loop and track_host visit them so; tests/host_track_check.cpp holds both forms
// against each other).
SUSHI_GEOM_HD inline bool track_replaces_in_order(double v, double best) { return v < best; }

// D_e[j] from near_e[j], u_e[j] and jump_e = m_{e-1} + penalty.  *move: the winning d, or TRACK_JUMP; a tie moves.
SUSHI_GEOM_HD inline double track_step(double near, int32_t d, double u, double jump, int16_t* move) {
    const bool take_near = near <= jump;
    *move = take_near ? (int16_t)d : TRACK_JUMP;
    return u + (take_near ? near : jump);
}

// ---- the host side of a call ----
// The axis is cut as the segmentation pass cuts it (axis_core.hpp), with a threshold of its own: a work item also stages a halo of
// reach_e values on each side of its PER * 256, so the small items are kept as long as the segmentation pass keeps them.
constexpr int64_t TRACK_FILL = 1024;
constexpr int TRACK_THREADS = AXIS_THREADS;

inline PathSplit track_split(int32_t n_shift) {
    PathSplit s;
    s.per = axis_per(axis_items(n_shift, AXIS_PER_LARGE), TRACK_FILL);
    s.n_items = axis_items(n_shift, s.per);
    s.grid = axis_grid(s.n_items);
    return s;
}

// workspace: path_layout's two sets of partial records (one record per workgroup of the grid), for track_split's grid
inline PathLayout track_layout(int32_t n_shift) { return path_layout_of(track_split(n_shift).grid); }
inline size_t track_layout_bytes(int n_rows, int64_t n_shift) {
    return n_rows < 1 || n_shift < 1 || n_shift > INT32_MAX ? 0 : track_layout((int32_t)n_shift).bytes;
}

// a launch's halo is loaded in rounds of one value per thread; the kernels are instantiated for 0, 2 and 8 rounds (reach 0, reach
// <= 256, reach <= TRACK_MAX_REACH)
constexpr int TRACK_HALO_SMALL = 2, TRACK_HALO_LARGE = 2 * TRACK_MAX_REACH / TRACK_THREADS;
SUSHI_GEOM_HD inline int track_halo_rounds(int32_t reach) {
    return reach == 0 ? 0 : (2 * reach <= TRACK_HALO_SMALL * TRACK_THREADS ? TRACK_HALO_SMALL : TRACK_HALO_LARGE);
}
// bytes of LDS a launch stages: its PER * 256 values of D_{e-1} and reach_e on each side (none at reach 0: every candidate is the
// thread's own value)
inline size_t track_tile_bytes(int per, int32_t reach) { return reach == 0 ? 0 : ((size_t)per * TRACK_THREADS + 2 * (size_t)reach) * 8; }

// ---- the wide form of a call (include/sushi_hip.h "wide tracking"; its arithmetic: track_wide_core.hpp) ----
constexpr int32_t TRACK_WIDE_MAX_REACH = SUSHI_HIP_TRACK_WIDE_MAX_REACH;
static_assert(TRACK_WIDE_MAX_REACH == INT16_MAX, "a move word holds every wide move, and TRACK_JUMP stays free");

// a window tile: WIDE_TILE consecutive indices from a multiple of WIDE_TILE on; an index inside it fits 16 bits
constexpr int WIDE_TILE_BITS = 10;
constexpr int32_t WIDE_TILE = 1 << WIDE_TILE_BITS;
static_assert(TRACK_MAX_REACH + 1 >= WIDE_TILE, "every wide reach is at least a tile: a window that the axis does not cut spans a boundary");

SUSHI_GEOM_HD inline int64_t wide_tiles(int64_t n_shift) { return (n_shift + WIDE_TILE - 1) >> WIDE_TILE_BITS; }
SUSHI_GEOM_HD inline bool wide_row(int32_t reach) { return reach > TRACK_MAX_REACH; }
SUSHI_GEOM_HD inline bool wide_step_cost_ok(double step_cost) { return step_cost == 0.0; }          // +0.0 or -0.0

// workspace of a wide call: the plain call's layout, then the records of one row -- [pv: f64 x n_shift][sv: f64 x n_shift]
// [pi: u32 x n_shift][si: u32 x n_shift], each array padded to 256 bytes.  One row's records live at a time: a wide row's tile pass
// writes them and its step reads them, in stream order.
struct WideLayout {
    size_t pv, sv, pi, si, bytes;           // offsets from the workspace's start
};
inline WideLayout wide_layout_of(size_t plain_bytes, int32_t n_shift) {
    WideLayout l;
    l.pv = align_up(plain_bytes, 256);
    l.sv = l.pv + align_up(8 * (size_t)n_shift, 256);
    l.pi = l.sv + align_up(8 * (size_t)n_shift, 256);
    l.si = l.pi + align_up(4 * (size_t)n_shift, 256);
    l.bytes = l.si + align_up(4 * (size_t)n_shift, 256);
    return l;
}
inline size_t track_wide_layout_bytes(int n_rows, int64_t n_shift) {
    const size_t plain = track_layout_bytes(n_rows, n_shift);
    return plain == 0 ? 0 : wide_layout_of(plain, (int32_t)n_shift).bytes;
}
// the tile pass's grid: one workgroup per window tile, at most AXIS_MAX_GRID of them striding over the tiles
inline unsigned wide_tile_grid(int32_t n_shift) { return axis_grid(wide_tiles(n_shift)); }

// ---- staging: a call's arguments -> a refusal, or the facts of its launches ----
// What the four walks (forward and margins, plain and ordered) stage alike; `wide` is the entry point's, not the rows': it selects
// the reach's bound and the workspace a call must bring.
struct TrackCall {
    PathSplit split;
    WideLayout wide;            // the wide layout behind the walk's own: what a wide call's workspace holds
    unsigned tile_grid;
    int n_wide;                 // rows of the call that go through the wide kernels (0 unless `wide`)
};

// EINVAL, what every walk refuses first: a null table or workspace; an unknown method; n_rows < 1, n_shift < 1, n_curve < 1, n_shift
// > n_curve; row0 < 0, n_total < 1 or rows row0 .. row0 + n_rows - 1 not inside [0, n_total) (no sum that could pass int is formed);
// a penalty or a step_cost that is not finite or is negative
inline int track_args_check(const void* rows, const void* reach, const void* mem, int n_rows, int32_t n_shift, int64_t n_curve,
                            int method, double penalty, double step_cost, int row0, int n_total) {
    if (!rows || !reach || !mem) return SUSHI_HIP_EINVAL;
    if (!method_known(method)) return SUSHI_HIP_EINVAL;
    if (n_rows < 1 || n_shift < 1 || n_curve < 1 || n_shift > n_curve) return SUSHI_HIP_EINVAL;
    if (n_total < 1 || row0 < 0 || row0 >= n_total || n_rows > n_total - row0) return SUSHI_HIP_EINVAL;
    if (!isfinite(penalty) || penalty < 0.0 || !isfinite(step_cost) || step_cost < 0.0) return SUSHI_HIP_EINVAL;
    return SUSHI_HIP_OK;
}
// a used reach: inside 0 .. TRACK_MAX_REACH (wide: TRACK_WIDE_MAX_REACH), and above TRACK_MAX_REACH only beside a step_cost of
// +-0.0; such a row is counted
inline bool track_reach_ok(int32_t reach, double step_cost, bool wide, int& n_wide) {
    if (reach < 0 || reach > (wide ? TRACK_WIDE_MAX_REACH : TRACK_MAX_REACH)) return false;
    if (wide_row(reach)) {
        if (!wide_step_cost_ok(step_cost)) return false;
        ++n_wide;
    }
    return true;
}
// the forward walks' EINVALs: track_args_check's; a row that leaves the curve buffer (no sum is formed) or a weight that is not
// finite or is negative; a reach that is not track_reach_ok in any row but the sequence's row 0 (whose reach is ignored)
inline int track_rows_check(const SushiHipJointRow* rows, const int32_t* reach, const void* mem, int n_rows, int32_t n_shift,
                            int64_t n_curve, int method, double penalty, double step_cost, int row0, int n_total, bool wide, int& n_wide) {
    const int rc = track_args_check(rows, reach, mem, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total);
    if (rc != SUSHI_HIP_OK) return rc;
    n_wide = 0;
    for (int i = 0; i < n_rows; ++i) {
        if (!axis_row_ok(rows[i], n_curve, n_shift)) return SUSHI_HIP_EINVAL;
        if ((row0 > 0 || i > 0) && !track_reach_ok(reach[i], step_cost, wide, n_wide)) return SUSHI_HIP_EINVAL;
    }
    return SUSHI_HIP_OK;
}
// what every walk does last: the split, and the workspace -- `plain_bytes` the walk's own layout's, the wide layout behind it.
// EALIGN: a workspace that is not 256-byte aligned; ENOSPACE: mem_bytes below the layout's (wide: the wide layout's).
inline int track_workspace_check(const void* mem, size_t mem_bytes, size_t plain_bytes, int32_t n_shift, bool wide, TrackCall& out) {
    out.split = track_split(n_shift);
    out.wide = wide_layout_of(plain_bytes, n_shift);
    out.tile_grid = wide_tile_grid(n_shift);
    if ((uintptr_t)mem & 255) return SUSHI_HIP_EALIGN;
    if (mem_bytes < (wide ? out.wide.bytes : plain_bytes)) return SUSHI_HIP_ENOSPACE;
    return SUSHI_HIP_OK;
}

struct TrackStage : TrackCall {
    PathLayout lay;
};

// track_rows_check's refusals, then track_workspace_check's.  `out` is unspecified after a refusal.
inline int stage_track(const SushiHipJointRow* rows, const int32_t* reach, int n_rows, int32_t n_shift, int64_t n_curve, int method,
                       double penalty, double step_cost, int row0, int n_total, const void* mem, size_t mem_bytes, TrackStage& out,
                       bool wide = false) {
    const int rc = track_rows_check(rows, reach, mem, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total, wide, out.n_wide);
    if (rc != SUSHI_HIP_OK) return rc;
    out.lay = track_layout(n_shift);
    return track_workspace_check(mem, mem_bytes, out.lay.bytes, n_shift, wide, out);
}

// ---- the backtrack: one walker, on the device (one lane) and on the CPU ----
// s_{E-1} = a_{E-1}; s_{e-1} = move_e[s_e] == TRACK_JUMP ? a_{e-1} : s_e + move_e[s_e], clamped into the axis
SUSHI_GEOM_HD inline void track_backtrack(const int16_t* move, const int32_t* row_arg, int n_total, int32_t n_shift, int32_t* out_shift) {
    int32_t s = path_clamp(row_arg[n_total - 1], n_shift);
    out_shift[n_total - 1] = s;
    for (int e = n_total - 1; e >= 1; --e) {
        const int16_t m = move[(int64_t)e * n_shift + s];
        // (|m| <= TRACK_MAX_REACH where the forward pass wrote it; any other word is clamped as well: 64 bits, no overflow)
        const int64_t to = (int64_t)s + m;
        s = m == TRACK_JUMP ? path_clamp(row_arg[e - 1], n_shift) : (int32_t)(to < 0 ? 0 : (to >= n_shift ? n_shift - 1 : to));
        out_shift[e - 1] = s;
    }
}

}  // namespace sushi
#endif
