// sushi_amd/csrc/sushi_track.hip -- the tracking pass, a shift that wanders from event to event (gfx950): sushi_hip_track_forward,
// _forward_keep (the same launches with every row of D kept), sushi_hip_track_backtrack, sushi_hip_track_margins (the pass's
// min-marginals), and the _wide form of each walk, with a reach of up to TRACK_WIDE_MAX_REACH = 32767 where moves are free.
//
// The rows of a sequence (sushi_hip_match_curves output, each from a curve_off of its own) lie on one shift axis in event order.
// Between consecutive rows the shift may move by at most reach_e samples at step_cost a sample, or jump anywhere at `penalty`:
// D_e[j] = u_e[j] + min(min_{|d| <= reach_e} (D_{e-1}[j + d] + step_cost |d|), m_{e-1} + penalty), in the arithmetic
// include/sushi_hip.h states and track_core.hpp implements (float64, products and sums rounded separately: this unit is compiled
// with -ffp-contract=off).  The output is bit-identical to the NumPy restatement (sushi_amd/track.py track_host); with every reach 0
// it is the segmentation pass (sushi_path.hip).
//
// One plain launch per row, stream-ordered, as in sushi_path.hip: the launch boundary is the pass's only all-to-all (m_{e-1}), which
// travels as one partial record per workgroup (path_device.hpp), and no grid waits on itself.  D lives in two halves: row e reads
// half (e - 1) & 1 -- other work items' indices as well -- and writes half e & 1.  Thread t of a work item holds the shift indices t,
// t + 256, ...: lane <-> consecutive index.  The hot part is the window minimum: a work item stages its PER x 256 values of D_{e-1}
// and reach_e values on each side once into LDS, and every candidate but the thread's own (d = 0) is read from there -- for one d a
// wave reads 64 consecutive doubles -- in the order -1, +1, -2, +2, ..., in which the tie rule is a strict comparison.  A row's
// curve_off, weight and reach are arguments of its launch: nothing is uploaded.
//
// The margins: M_e[j] is the cost of the best whole path that puts event e at shift j, the forward pass's D_e[j]
// (kept by sushi_hip_track_forward_keep) plus B_e[j], what the events after e add.  B comes from the same recurrence run from the
// last row down: C_e[j] = u_e[j] + B_e[j], B_e[j] = min(min_{|d| <= reach_{e+1}} (C_{e+1}[j + d] + step_cost |d|), n_{e+1} + penalty)
// (track_margin_core.hpp; bit-identical to track.py track_margins_host).  The shape is the forward walk's, from the call's last row
// down; C lives in two halves (row e reads half (e + 1) & 1 and writes half e & 1).  Beside the window minimum a thread reads
// D_e[j], forms M and C, and the workgroup leaves one partial record of three first minima -- of C, of M, and of M outside the
// guard window around s_e (the backtrack's output: read from device memory, workgroup-uniform) -- which the next launch reduces
// before anything else; the thread that owns s_e stores through_e.  No grid waits on itself, and there are no atomics.
//
// The wide calls: a row whose reach is at most TRACK_MAX_REACH goes through the step kernels above (the same code,
// the same launches, so the same bits).  A wider row -- its step_cost is +-0.0: stage_track -- takes two stream-ordered launches,
// with no grid-wide wait and no atomics:
//   wide_tile_kernel     (sushi_track_wide_tile.inc, shared with sushi_track_order.hip) one workgroup per window tile of WIDE_TILE
//                        = 1024 values of the row before (D_{e-1}; C_{e+1} backwards), read once: a thread holds four consecutive
//                        values, scans them, the wave scans the threads' totals by shuffles, the four waves' totals cross through
//                        LDS; per element it writes the record of the tile's values up to it and of those from it on (value; first
//                        and last index that attain it, 16 bits each);
//   wide_*_step_kernel   track_step_kernel's / margin_step_kernel's shape -- the same work items, lane <-> consecutive index, the
//                        same partial records, m_{e-1} reduced through path_device.hpp -- but near_e[j] is track_wide_core.hpp's
//                        wide_near: per side one suffix record, one prefix record and the whole tiles between, whose records (the
//                        prefix at each tile's last element: at most WIDE_ITEM_TILES = 67) the work item stages in LDS once; of a
//                        wave's lanes nearly all ask for the same tiles, so those reads are broadcasts.
// A shift costs a few records and at most 2 * reach / 1024 LDS reads instead of 2 * reach candidates.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "track_core.hpp"
#include "track_margin_core.hpp"
#include "track_wide_core.hpp"
#include "path_device.hpp"
#include "track_margin_device.hpp"

namespace {

using namespace sushi;

#include "sushi_track_step.inc"             // TrackArgs, track_step_kernel, track_close_kernel, launch_step
#include "sushi_track_margins_step.inc"     // MarginArgs, margin_step_kernel, margin_close_kernel, launch_margin_step

#include "sushi_track_wide_tile.inc"         // wide_tile_kernel, launch_wide_tiles, WideItemTiles, StagedTiles, stage_item_tiles

// one wave; lane 0 walks the rows backwards: every step reads the move the step before it chose
__global__ __launch_bounds__(64)
void track_backtrack_kernel(const int16_t* move, const int32_t* row_arg, int n_total, int32_t n_shift, int32_t* out_shift) {
    if (threadIdx.x == 0 && blockIdx.x == 0) track_backtrack(move, row_arg, n_total, n_shift, out_shift);
}

// ---- the steps ----
template <int PER, bool MAX>
__global__ __launch_bounds__(TRACK_THREADS)
void wide_track_step_kernel(TrackArgs a, WideRecords w) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    __shared__ WideItemTiles staged;
    const float* __restrict__ row = a.row;
    const double* __restrict__ Din = a.D_in;
    double* __restrict__ Dout = a.D_out;
    int16_t* __restrict__ move = a.move;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = a.reach;
    double jump = 0.0;                      // (a wide row is never the sequence's row 0: its reach is 0)
    if (a.prev == PREV_PARTIALS) jump = reduce_partials<METHOD>(a.in, a.n_partials, blockIdx.x == 0, a.e - 1, a, lds) + a.penalty;
    else if (a.prev == PREV_ROW_MIN) jump = a.row_min[a.e - 1] + a.penalty;

    MinD best = {INFINITY, PATH_NO_INDEX};
    OwnF own = {own_worst<METHOD>(), PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        const StagedTiles tiles = stage_item_tiles(w, base, SPAN, reach, n_shift, staged);
        int32_t at[PER];
        float r[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) at[p] = axis_at(j0 + p * TRACK_THREADS, n_shift);
#pragma unroll
        for (int p = 0; p < PER; ++p) r[p] = row[at[p]];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            // (an index past the axis's end computes the last one's window, and stores nothing)
            int32_t nd = 0;
            const double near = wide_near(Din, w.pv, w.sv, w.pi, w.si, tiles, at[p], n_shift, reach, a.step_cost, &nd);
            const double u = path_cost(METHOD, a.weight, r[p]);
            int16_t mv = 0;
            const double dn = track_step(near, nd, u, jump, &mv);
            const bool take = (int)valid & (int)path_min_replaces(dn, (int32_t)j, best.v, best.i);
            best.v = take ? dn : best.v; best.i = take ? (int32_t)j : best.i;
            const bool take_own = (int)valid & (int)path_own_replaces(METHOD, r[p], (int32_t)j, own.v, own.i);
            own.v = take_own ? r[p] : own.v; own.i = take_own ? (int32_t)j : own.i;
            if (valid) {
                Dout[j] = dn;
                move[j] = mv;
            }
        }
    }
    best = block_first_min(best, lds);
    own = block_first_own<METHOD>(own, lds);
    if (threadIdx.x == 0) {
        a.out.d_min[blockIdx.x] = best.v; a.out.d_arg[blockIdx.x] = best.i;
        a.out.own_idx[blockIdx.x] = own.i; a.out.own_val[blockIdx.x] = own.v;
    }
}

template <int PER, bool MAX>
__global__ __launch_bounds__(TRACK_THREADS)
void wide_margin_step_kernel(MarginArgs a, WideRecords w) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    __shared__ WideItemTiles staged;
    const float* __restrict__ row = a.row;
    const double* __restrict__ Cin = a.C_in;
    const double* __restrict__ Drow = a.D_row;
    double* __restrict__ Cout = a.C_out;
    double* __restrict__ Mrow = a.M_row;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = a.reach;
    const int32_t s_e = path_clamp(a.shift[a.e], n_shift);
    const int32_t guard = a.guard;
    double jump = 0.0;                      // (a wide row is never the sequence's last row: the reach after it is 0)
    if (a.prev == PREV_PARTIALS) jump = reduce_margin_partials(a, blockIdx.x == 0, a.e + 1, lds) + a.penalty;
    else if (a.prev == PREV_ROW_MIN) jump = a.c_min[a.e + 1] + a.penalty;

    MinD best_c = {INFINITY, PATH_NO_INDEX}, best_m = {INFINITY, PATH_NO_INDEX}, best_a = {INFINITY, PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        const StagedTiles tiles = stage_item_tiles(w, base, SPAN, reach, n_shift, staged);
        int32_t at[PER];
        float r[PER];
        double dd[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) at[p] = axis_at(j0 + p * TRACK_THREADS, n_shift);
#pragma unroll
        for (int p = 0; p < PER; ++p) dd[p] = Drow[at[p]];
#pragma unroll
        for (int p = 0; p < PER; ++p) r[p] = row[at[p]];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            int32_t nd = 0;
            const double near = wide_near(Cin, w.pv, w.sv, w.pi, w.si, tiles, at[p], n_shift, reach, a.step_cost, &nd);
            const double u = path_cost(METHOD, a.weight, r[p]);
            const double b = margin_back(near, jump);
            const double m = margin_through(dd[p], b, false);
            const double cn = margin_suffix(u, b, false);
            const bool take_c = (int)valid & (int)path_min_replaces(cn, (int32_t)j, best_c.v, best_c.i);
            best_c.v = take_c ? cn : best_c.v; best_c.i = take_c ? (int32_t)j : best_c.i;
            const bool take_m = (int)valid & (int)path_min_replaces(m, (int32_t)j, best_m.v, best_m.i);
            best_m.v = take_m ? m : best_m.v; best_m.i = take_m ? (int32_t)j : best_m.i;
            const bool take_a = (int)valid & (int)margin_outside(j, s_e, guard) & (int)path_min_replaces(m, (int32_t)j, best_a.v, best_a.i);
            best_a.v = take_a ? m : best_a.v; best_a.i = take_a ? (int32_t)j : best_a.i;
            if (valid) {
                Cout[j] = cn;
                if (Mrow) Mrow[j] = m;
                if (j == s_e) a.through[a.e] = m;
            }
        }
    }
    best_c = block_first_min(best_c, lds);
    best_m = block_first_min(best_m, lds);
    best_a = block_first_min(best_a, lds);
    if (threadIdx.x == 0) {
        a.out.c_min[blockIdx.x] = best_c.v; a.out.c_arg[blockIdx.x] = best_c.i;
        a.out.m_min[blockIdx.x] = best_m.v; a.out.m_arg[blockIdx.x] = best_m.i;
        a.out.a_min[blockIdx.x] = best_a.v; a.out.a_arg[blockIdx.x] = best_a.i;
    }
}


// ---- the drivers: one body per walk ----
// The forward walk.  keep: D_dev holds every row ([n_total][n_shift]: row e reads row e - 1 and writes row e) instead of two halves
// used by turns; the launches, and so the bits, are the same.  wide: the entry point is a wide one -- stage_track takes the wide
// bound and asks for the wide workspace, and a row of a reach above TRACK_MAX_REACH goes through the tile pass and the wide step
// (a plain call has no such row: stage_track refused it).
int track_forward(bool keep, bool wide, const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                  const int32_t* reach_host, int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0,
                  int n_total, double* D_dev, int16_t* move_dev, double* row_min_dev, int32_t* row_arg_dev, int32_t* row_own_index_dev,
                  float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    if (!curves_dev || !rows_host || !reach_host || !D_dev || !move_dev || !row_min_dev || !row_arg_dev || !row_own_index_dev ||
        !row_own_score_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    TrackStage staged;
    const int rc = stage_track(rows_host, reach_host, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total, mem_dev,
                               mem_bytes, staged, wide);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_dev | (uintptr_t)row_min_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)row_arg_dev | (uintptr_t)row_own_index_dev | (uintptr_t)row_own_score_dev) & 3) ||
        ((uintptr_t)move_dev & 1))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    const PathSplit& split = staged.split;
    const WideRecords w = wide_records((char*)mem_dev, staged.wide);
    TrackArgs a;
    a.penalty = penalty;
    a.step_cost = step_cost;
    a.n_shift = n_shift;
    a.n_items = split.n_items;
    a.n_partials = (int)split.grid;
    a.row_min = row_min_dev; a.row_arg = row_arg_dev; a.row_own_index = row_own_index_dev; a.row_own_score = row_own_score_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(split.grid), block(TRACK_THREADS);
    for (int i = 0; i < n_rows; ++i) {
        a.e = row0 + i;
        a.row = curves_dev + rows_host[i].curve_off;
        a.weight = rows_host[i].weight;
        a.reach = a.e == 0 ? 0 : reach_host[i];
        // (row 0 has no row before it: its launch's loads of D_in, which are always made and never used, go to its own row)
        a.D_in = D_dev + (keep ? (int64_t)(a.e == 0 ? 0 : a.e - 1) : (int64_t)((a.e + 1) & 1)) * n_shift;
        a.D_out = D_dev + (keep ? (int64_t)a.e : (int64_t)(a.e & 1)) * n_shift;
        a.move = move_dev + (int64_t)a.e * n_shift;
        a.prev = a.e == 0 ? PREV_NONE : (i == 0 ? PREV_ROW_MIN : PREV_PARTIALS);
        a.in = partial_set((char*)mem_dev, staged.lay, (i + 1) & 1);
        a.out = partial_set((char*)mem_dev, staged.lay, i & 1);
        if (wide_row(a.reach)) {
            launch_wide_tiles(a.D_in, n_shift, staged.tile_grid, w, st);
            if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
            axis_dispatch(split.per, mx, [&](auto per, auto is_max) {
                hipLaunchKernelGGL((wide_track_step_kernel<per.value, is_max.value>), grid, block, 0, st, a, w);
            });
        } else {
            const int halo = track_halo_rounds(a.reach);
            const size_t tile_bytes = track_tile_bytes(split.per, a.reach);
            axis_dispatch(split.per, mx, [&](auto per, auto is_max) {
                launch_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
            });
        }
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    a.e = row0 + n_rows - 1;
    a.in = partial_set((char*)mem_dev, staged.lay, (n_rows - 1) & 1);
    if (mx) hipLaunchKernelGGL(track_close_kernel<true>, dim3(1), block, 0, st, a);
    else hipLaunchKernelGGL(track_close_kernel<false>, dim3(1), block, 0, st, a);
    return launch_ok();
}

// The margins walk, from the call's last row down.  wide: as track_forward's -- stage_margins' bound and workspace, and a row
// whose step into the row after it has a reach above TRACK_MAX_REACH goes through the tile pass (over C_{e+1}) and the wide step.
int track_margins(bool wide, const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                  const int32_t* guard_host, int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0,
                  int n_total, const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* c_min_dev, double* through_dev,
                  double* best_dev, int32_t* best_arg_dev, double* alt_dev, int32_t* alt_arg_dev, double* M_dev, void* mem_dev,
                  size_t mem_bytes, void* hip_stream) {
    if (!curves_dev || !rows_host || !reach_host || !guard_host || !D_all_dev || !shift_dev || !C_dev || !c_min_dev || !through_dev ||
        !best_dev || !best_arg_dev || !alt_dev || !alt_arg_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    MarginStage staged;
    const int rc = stage_margins(rows_host, reach_host, guard_host, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total,
                                 mem_dev, mem_bytes, staged, wide);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_all_dev | (uintptr_t)C_dev | (uintptr_t)c_min_dev | (uintptr_t)through_dev | (uintptr_t)best_dev |
          (uintptr_t)alt_dev | (uintptr_t)M_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)shift_dev | (uintptr_t)best_arg_dev | (uintptr_t)alt_arg_dev) & 3))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    const PathSplit& split = staged.split;
    const WideRecords w = wide_records((char*)mem_dev, staged.wide);
    MarginArgs a;
    a.penalty = penalty;
    a.step_cost = step_cost;
    a.shift = shift_dev;
    a.n_shift = n_shift;
    a.n_items = split.n_items;
    a.n_partials = (int)split.grid;
    a.through = through_dev; a.best = best_dev; a.best_arg = best_arg_dev; a.alt = alt_dev; a.alt_arg = alt_arg_dev; a.c_min = c_min_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(split.grid), block(TRACK_THREADS);
    int turn = 0;                           // the launches of the call, counted: which record set a launch writes
    for (int i = n_rows - 1; i >= 0; --i, ++turn) {
        a.e = row0 + i;
        a.row = curves_dev + rows_host[i].curve_off;
        a.weight = rows_host[i].weight;
        a.reach = margin_reach_after(reach_host, i, n_rows, staged.first_call);
        a.guard = guard_host[i];
        a.C_in = C_dev + (int64_t)((a.e + 1) & 1) * n_shift;
        a.C_out = C_dev + (int64_t)(a.e & 1) * n_shift;
        a.D_row = D_all_dev + (int64_t)a.e * n_shift;
        a.M_row = M_dev ? M_dev + (int64_t)a.e * n_shift : nullptr;
        a.prev = a.e == n_total - 1 ? PREV_NONE : (turn == 0 ? PREV_ROW_MIN : PREV_PARTIALS);
        a.in = margin_set((char*)mem_dev, staged.lay, (turn + 1) & 1);
        a.out = margin_set((char*)mem_dev, staged.lay, turn & 1);
        if (wide_row(a.reach)) {
            launch_wide_tiles(a.C_in, n_shift, staged.tile_grid, w, st);
            if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
            axis_dispatch(split.per, mx, [&](auto per, auto is_max) {
                hipLaunchKernelGGL((wide_margin_step_kernel<per.value, is_max.value>), grid, block, 0, st, a, w);
            });
        } else {
            const int halo = track_halo_rounds(a.reach);
            const size_t tile_bytes = track_tile_bytes(split.per, a.reach);
            axis_dispatch(split.per, mx, [&](auto per, auto is_max) {
                launch_margin_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
            });
        }
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    a.e = row0;
    a.in = margin_set((char*)mem_dev, staged.lay, (n_rows - 1) & 1);
    hipLaunchKernelGGL(margin_close_kernel, dim3(1), block, 0, st, a);
    return launch_ok();
}

}  // namespace

extern "C" {

size_t sushi_hip_track_bytes(int n_rows, int32_t n_shift) { return track_layout_bytes(n_rows, n_shift); }
size_t sushi_hip_track_margins_bytes(int n_rows, int32_t n_shift) { return margin_layout_bytes(n_rows, n_shift); }
size_t sushi_hip_track_wide_bytes(int n_rows, int32_t n_shift) { return track_wide_layout_bytes(n_rows, n_shift); }
size_t sushi_hip_track_margins_wide_bytes(int n_rows, int32_t n_shift) { return margin_wide_layout_bytes(n_rows, n_shift); }

// the entry points: track_forward(keep, wide), track_margins(wide)
int sushi_hip_track_forward(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                            int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0, int n_total,
                            double* D_dev, int16_t* move_dev, double* row_min_dev, int32_t* row_arg_dev, int32_t* row_own_index_dev,
                            float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward(false, false, curves_dev, n_curve, rows_host, reach_host, n_rows, n_shift, method, penalty, step_cost, row0,
                             n_total, D_dev, move_dev, row_min_dev, row_arg_dev, row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes,
                             hip_stream);
}); }

int sushi_hip_track_forward_keep(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                 int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0, int n_total,
                                 double* D_all_dev, int16_t* move_dev, double* row_min_dev, int32_t* row_arg_dev, int32_t* row_own_index_dev,
                                 float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward(true, false, curves_dev, n_curve, rows_host, reach_host, n_rows, n_shift, method, penalty, step_cost, row0,
                             n_total, D_all_dev, move_dev, row_min_dev, row_arg_dev, row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes,
                             hip_stream);
}); }

int sushi_hip_track_forward_wide(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                 int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0, int n_total,
                                 double* D_dev, int16_t* move_dev, double* row_min_dev, int32_t* row_arg_dev, int32_t* row_own_index_dev,
                                 float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward(false, true, curves_dev, n_curve, rows_host, reach_host, n_rows, n_shift, method, penalty, step_cost, row0,
                             n_total, D_dev, move_dev, row_min_dev, row_arg_dev, row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes,
                             hip_stream);
}); }

int sushi_hip_track_forward_wide_keep(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                      int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0, int n_total,
                                      double* D_all_dev, int16_t* move_dev, double* row_min_dev, int32_t* row_arg_dev, int32_t* row_own_index_dev,
                                      float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward(true, true, curves_dev, n_curve, rows_host, reach_host, n_rows, n_shift, method, penalty, step_cost, row0,
                             n_total, D_all_dev, move_dev, row_min_dev, row_arg_dev, row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes,
                             hip_stream);
}); }

int sushi_hip_track_margins(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                            const int32_t* guard_host, int n_rows, int32_t n_shift, int method, double penalty, double step_cost,
                            int row0, int n_total, const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* c_min_dev,
                            double* through_dev, double* best_dev, int32_t* best_arg_dev, double* alt_dev, int32_t* alt_arg_dev,
                            double* M_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_margins(false, curves_dev, n_curve, rows_host, reach_host, guard_host, n_rows, n_shift, method, penalty, step_cost,
                             row0, n_total, D_all_dev, shift_dev, C_dev, c_min_dev, through_dev, best_dev, best_arg_dev, alt_dev,
                             alt_arg_dev, M_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_margins_wide(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                 const int32_t* guard_host, int n_rows, int32_t n_shift, int method, double penalty, double step_cost,
                                 int row0, int n_total, const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* c_min_dev,
                                 double* through_dev, double* best_dev, int32_t* best_arg_dev, double* alt_dev, int32_t* alt_arg_dev,
                                 double* M_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_margins(true, curves_dev, n_curve, rows_host, reach_host, guard_host, n_rows, n_shift, method, penalty, step_cost,
                             row0, n_total, D_all_dev, shift_dev, C_dev, c_min_dev, through_dev, best_dev, best_arg_dev, alt_dev,
                             alt_arg_dev, M_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_backtrack(const int16_t* move_dev, const int32_t* row_arg_dev, int n_total, int32_t n_shift,
                              int32_t* out_shift_dev, void* hip_stream) { return c_boundary([&]() -> int {
    if (!move_dev || !row_arg_dev || !out_shift_dev || n_total < 1 || n_shift < 1) return SUSHI_HIP_EINVAL;
    if (((uintptr_t)move_dev & 1) || (((uintptr_t)row_arg_dev | (uintptr_t)out_shift_dev) & 3)) return SUSHI_HIP_EALIGN;
    hipLaunchKernelGGL(track_backtrack_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, move_dev, row_arg_dev, n_total, n_shift,
                       out_shift_dev);
    return launch_ok();
}); }

}  // extern "C"
