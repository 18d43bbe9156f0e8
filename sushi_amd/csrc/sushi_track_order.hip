// sushi_amd/csrc/sushi_track_order.hip -- the tracking pass (sushi_track.hip) with events kept in order -- a jump into (e, j) comes
// from an index of row e - 1 no further than back_e above j, at a penalty of row e's own (gfx950): sushi_hip_track_forward_ordered,
// _ordered_keep (the same launches with every row of D kept), sushi_hip_track_backtrack_ordered, sushi_hip_track_order_margins (the
// ordered pass's min-marginals), and the _wide form of each walk, with a reach of up to TRACK_WIDE_MAX_REACH = 32767 where moves are
// free.
//
// D_e[j] = u_e[j] + min(near_e[j], P_{e-1}[t_e(j)] + penalty_e), P the prefix minimum of D_{e-1} and t_e(j) = min(j + back_e,
// n_shift - 1), in the arithmetic include/sushi_hip.h "ordered tracking" states and track_core.hpp / track_order_core.hpp implement
// (float64, -ffp-contract=off).  The output is bit-identical to the NumPy restatement (sushi_amd/track.py track_ordered_host); with
// every back unlimited and one penalty it is sushi_track.hip's, bit for bit.
//
// Per row the all-to-all is no longer one scalar but a whole row, P_{e-1}, and with it A_{e-1}, the index that attains it.  Three
// plain launches per row, stream-ordered; the launch boundary is the only synchronisation, and no workgroup waits on another:
//   step   sushi_track.hip's step kernel -- the window minimum over an LDS tile, the <PER, MAX, HALO> dispatch, the partial records
//          -- with jump read per index from P at t_e(j): lane <-> consecutive index still, so a wave reads 64 consecutive doubles
//          shifted by back_e.  It also leaves one (min, first index) record per work item.
//   scan   one workgroup: the exclusive scan of the work items' records -- what lies before every item -- and the row's outputs
//          from the partial records (so no launch closes a call).
//   apply  a work item re-reads its PER x 256 values of D_e, scans them (a wave's shuffles, the four waves through LDS, PER rounds
//          in index order) onto what lies before it, and writes P_e and A_e.
// P is one buffer: row e's step reads P_{e-1} before row e's apply writes P_e.  A call that ends before the sequence's last row
// leaves P and A of its last row in the state, and the next call's first step reads them: chunks have the bits of one call.
//
// The margins: M_e[j] = D_e[j] + B_e[j], D the ordered forward pass's rows (kept by
// sushi_hip_track_forward_ordered_keep) and B what the events after e add: B_e[j] = min(nearB[j], S_{e+1}[t'_e(j)] + penalty_{e+1}),
// nearB the window minimum over C_{e+1}, S_{e+1} the suffix minimum of C_{e+1} and t'_e(j) = max(j - back_{e+1}, 0); C_e[j] = u_e[j] +
// B_e[j] -- the arithmetic include/sushi_hip.h "ordered margins" states and track_margin_core.hpp / track_order_margin_core.hpp
// implement.  The output is bit-identical to the NumPy restatement (sushi_amd/track.py track_ordered_margins_host); with every back
// unlimited and one penalty it is sushi_track.hip's margins, bit for bit.  Three plain launches per row, from the call's last row
// down, stream-ordered; the launch boundary is the only synchronisation, and no workgroup waits on another:
//   step   sushi_track.hip's margins step kernel -- the window minimum over an LDS tile of C_{e+1}, the <PER, MAX, HALO> dispatch,
//          the partial records of three first minima, through_e -- with jumpB read per index from S at t'_e(j): lane <-> consecutive
//          index still, so a wave reads 64 consecutive doubles shifted down by the back.  It also leaves one (min, first index)
//          record of C_e per work item.
//   scan   one workgroup: the exclusive suffix scan of the work items' records -- what lies after every item -- and the row's outputs
//          from the partial records (so no launch closes a call).
//   apply  a work item re-reads its PER x 256 values of C_e, scans them downwards onto what lies after it, and writes S_e.  Only
//          values travel: adjacent spans met in index order need no index to keep the first of equal minima
//          (order_suffix_combine).  Every round's wave scan is done first; the PER x 4 wave totals cross the workgroup through LDS
//          behind one barrier, and every thread folds the totals after its own wave itself.
// S is one buffer: row e's step reads S_{e+1} before row e's apply writes S_e.  A call that ends above the sequence's row 0 leaves
// C and S of its last row in the state, and the next call's first step reads them: chunks have the bits of one call.
//
// The wide calls: a row whose reach is at most TRACK_MAX_REACH takes the three launches above (the same code, the
// same launches, so the same bits).  A wider row -- its step_cost is +-0.0: stage_track_ordered -- takes four stream-ordered
// launches, with no grid-wide wait and no atomics:
//   wide_tile_kernel          sushi_track.hip's tile pass (sushi_track_wide_tile.inc) over the row before (D_{e-1}; C_{e+1}
//                             backwards): per element the record of its 1024-value tile up to it and from it on;
//   wide_order_*step_kernel   wide_track_step_kernel's / wide_margin_step_kernel's shape -- the whole tiles' records staged in LDS
//                             once per work item, track_wide_core.hpp's wide_near, lane <-> consecutive index -- with the jump read
//                             per index: P_{e-1} at t_e(j) forwards, S_{e+1} at t'_e(j) backwards, asked for with the row's loads.
//                             It leaves the partial records and the per-work-item (min, first index) record the scan reads;
//   scan, apply               the ordered pass's own (order_scan_kernel / order_apply_kernel; order_margin_scan_kernel /
//                             order_margin_apply_kernel), as they are.
// The window minimum's bits are the candidate loop's and the jump term is the ordered pass's own expression, so
// every output has the bits of the ordered recurrence with the loop run to that reach.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "track_order_wide_core.hpp"            // track_order_core.hpp, track_order_margin_core.hpp, track_wide_core.hpp
#include "path_device.hpp"
#include "track_margin_device.hpp"

namespace {

using namespace sushi;

#include "sushi_track_order_step.inc"           // OrderArgs, order_step_kernel, order_scan_kernel, order_apply_kernel, launch_step
#include "sushi_track_order_margins_step.inc"   // OrderMarginArgs, order_margin_step_kernel, _scan_kernel, _apply_kernel, the launcher
#include "sushi_track_wide_tile.inc"            // wide_tile_kernel, launch_wide_tiles, WideItemTiles, StagedTiles, stage_item_tiles

// one wave; lane 0 walks the rows backwards: every step reads the move the step before it chose
__global__ __launch_bounds__(64)
void order_backtrack_kernel(const int16_t* move, const int32_t* from, const int32_t* back, const int32_t* row_arg, int n_total,
                            int32_t n_shift, int32_t* out_shift) {
    if (threadIdx.x == 0 && blockIdx.x == 0) order_backtrack(move, from, back, row_arg, n_total, n_shift, out_shift);
}

// order_step_kernel for a row of a reach above TRACK_MAX_REACH (never the sequence's row 0, whose reach is 0)
template <int PER, bool MAX>
__global__ __launch_bounds__(TRACK_THREADS)
void wide_order_step_kernel(OrderArgs a, WideRecords w) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    __shared__ WideItemTiles staged;
    const float* __restrict__ row = a.row;
    const double* __restrict__ Din = a.D_in;
    const double* __restrict__ Pin = a.P;
    double* __restrict__ Dout = a.D_out;
    int16_t* __restrict__ move = a.move;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = a.reach;

    MinD best = {INFINITY, PATH_NO_INDEX};
    OwnF own = {own_worst<METHOD>(), PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        // every load is always made, at an index inside the axis (axis_at; t_e(j) lies inside it for every j >= 0): P and the row
        // are asked for before the tiles are staged, and so before the first value is used
        int32_t at[PER];
        float r[PER];
        double pt[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) at[p] = axis_at(j0 + p * TRACK_THREADS, n_shift);
#pragma unroll
        for (int p = 0; p < PER; ++p) pt[p] = Pin[order_reach_back(at[p], a.back, n_shift)];
#pragma unroll
        for (int p = 0; p < PER; ++p) r[p] = row[at[p]];
        const StagedTiles tiles = stage_item_tiles(w, base, SPAN, reach, n_shift, staged);
        MinD mine = {INFINITY, PATH_NO_INDEX};
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            // (an index past the axis's end computes the last one's window, and stores nothing)
            int32_t nd = 0;
            const double near = wide_near(Din, w.pv, w.sv, w.pi, w.si, tiles, at[p], n_shift, reach, a.step_cost, &nd);
            const double u = path_cost(METHOD, a.weight, r[p]);
            int16_t mv = 0;
            const double dn = track_step(near, nd, u, order_jump(pt[p], a.penalty), &mv);
            const bool take = (int)valid & (int)path_min_replaces(dn, (int32_t)j, mine.v, mine.i);
            mine.v = take ? dn : mine.v; mine.i = take ? (int32_t)j : mine.i;
            const bool take_own = (int)valid & (int)path_own_replaces(METHOD, r[p], (int32_t)j, own.v, own.i);
            own.v = take_own ? r[p] : own.v; own.i = take_own ? (int32_t)j : own.i;
            if (valid) {
                Dout[j] = dn;
                move[j] = mv;
            }
        }
        // the item's record (valid in every thread), and the workgroup's over its items
        mine = block_first_min(mine, lds);
        if (threadIdx.x == 0) { a.item_min[item] = mine.v; a.item_arg[item] = mine.i; }
        const bool take = path_min_replaces(mine.v, mine.i, best.v, best.i);
        best.v = take ? mine.v : best.v; best.i = take ? mine.i : best.i;
    }
    own = block_first_own<METHOD>(own, lds);
    if (threadIdx.x == 0) {
        a.partials.d_min[blockIdx.x] = best.v; a.partials.d_arg[blockIdx.x] = best.i;
        a.partials.own_idx[blockIdx.x] = own.i; a.partials.own_val[blockIdx.x] = own.v;
    }
}

// order_margin_step_kernel for a row whose step into the row after it has a reach above TRACK_MAX_REACH (never the sequence's last
// row: there is no row after it)
template <int PER, bool MAX>
__global__ __launch_bounds__(TRACK_THREADS)
void wide_order_margin_step_kernel(OrderMarginArgs a, WideRecords w) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    __shared__ WideItemTiles staged;
    const float* __restrict__ row = a.row;
    const double* __restrict__ Cin = a.C_in;
    const double* __restrict__ Drow = a.D_row;
    const double* __restrict__ Sin = a.S;
    double* __restrict__ Cout = a.C_out;
    double* __restrict__ Mrow = a.M_row;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = a.reach;
    const int32_t s_e = path_clamp(a.shift[a.e], n_shift);
    const int32_t guard = a.guard;

    MinD best_c = {INFINITY, PATH_NO_INDEX}, best_m = {INFINITY, PATH_NO_INDEX}, best_a = {INFINITY, PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        // every load is always made, at an index inside the axis (t'_e(j) lies inside it for every j inside it): S, D_e and the
        // row are asked for before the tiles are staged
        int32_t at[PER];
        float r[PER];
        double dd[PER], st[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) at[p] = axis_at(j0 + p * TRACK_THREADS, n_shift);
#pragma unroll
        for (int p = 0; p < PER; ++p) st[p] = Sin[order_margin_from(at[p], a.back)];
#pragma unroll
        for (int p = 0; p < PER; ++p) dd[p] = Drow[at[p]];
#pragma unroll
        for (int p = 0; p < PER; ++p) r[p] = row[at[p]];
        const StagedTiles tiles = stage_item_tiles(w, base, SPAN, reach, n_shift, staged);
        MinD mine = {INFINITY, PATH_NO_INDEX};
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            int32_t nd = 0;
            const double near = wide_near(Cin, w.pv, w.sv, w.pi, w.si, tiles, at[p], n_shift, reach, a.step_cost, &nd);
            const double u = path_cost(METHOD, a.weight, r[p]);
            const double b = margin_back(near, order_margin_jump(st[p], a.penalty));
            const double m = margin_through(dd[p], b, false);
            const double cn = margin_suffix(u, b, false);
            const bool take_c = (int)valid & (int)path_min_replaces(cn, (int32_t)j, mine.v, mine.i);
            mine.v = take_c ? cn : mine.v; mine.i = take_c ? (int32_t)j : mine.i;
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
        // the item's record of C_e (valid in every thread), and the workgroup's over its items
        mine = block_first_min(mine, lds);
        if (threadIdx.x == 0) { a.item_min[item] = mine.v; a.item_arg[item] = mine.i; }
        const bool take = path_min_replaces(mine.v, mine.i, best_c.v, best_c.i);
        best_c.v = take ? mine.v : best_c.v; best_c.i = take ? mine.i : best_c.i;
    }
    best_m = block_first_min(best_m, lds);
    best_a = block_first_min(best_a, lds);
    if (threadIdx.x == 0) {
        a.in.c_min[blockIdx.x] = best_c.v; a.in.c_arg[blockIdx.x] = best_c.i;
        a.in.m_min[blockIdx.x] = best_m.v; a.in.m_arg[blockIdx.x] = best_m.i;
        a.in.a_min[blockIdx.x] = best_a.v; a.in.a_arg[blockIdx.x] = best_a.i;
    }
}

// ---- the drivers: one body per walk ----
// The forward walk.  keep: D_dev holds every row ([n_total][n_shift]: row e reads row e - 1 and writes row e) instead of two halves
// used by turns; the launches, and so the bits, are the same.  wide: the entry point is a wide one -- stage_track_ordered takes the
// wide bound and asks for the wide workspace, and a row of a reach above TRACK_MAX_REACH goes through the tile pass and the wide
// step in place of the step (a plain call has no such row: stage_track_ordered refused it).
int track_forward_ordered(bool keep, bool wide, const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                          const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                          const double* penalty_host, double step_cost, int row0, int n_total, double* D_dev, int16_t* move_dev,
                          double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                          int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    if (!curves_dev || !rows_host || !reach_host || !back_host || !penalty_host || !D_dev || !move_dev || !P_dev || !from_dev ||
        !back_dev || !row_min_dev || !row_arg_dev || !row_own_index_dev || !row_own_score_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    OrderStage staged;
    const int rc = stage_track_ordered(rows_host, reach_host, back_host, penalty_host, n_rows, n_shift, n_curve, method, step_cost, row0,
                                       n_total, mem_dev, mem_bytes, staged, wide);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_dev | (uintptr_t)P_dev | (uintptr_t)row_min_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)from_dev | (uintptr_t)back_dev | (uintptr_t)row_arg_dev | (uintptr_t)row_own_index_dev |
          (uintptr_t)row_own_score_dev) & 3) ||
        ((uintptr_t)move_dev & 1))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    char* mem = (char*)mem_dev;
    const PathSplit& split = staged.split;
    const OrderLayout& lay = staged.lay;
    const WideRecords w = wide_records(mem, staged.wide);
    OrderArgs a;
    a.step_cost = step_cost;
    a.P = P_dev;
    a.back_dev = back_dev;
    a.n_shift = n_shift;
    a.n_items = split.n_items;
    a.n_partials = (int)split.grid;
    a.partials = partial_set(mem, lay.partials, 0);
    a.item_min = (double*)(mem + lay.item_min); a.item_arg = (int32_t*)(mem + lay.item_arg);
    a.before_min = (double*)(mem + lay.before_min); a.before_arg = (int32_t*)(mem + lay.before_arg);
    a.row_min = row_min_dev; a.row_arg = row_arg_dev; a.row_own_index = row_own_index_dev; a.row_own_score = row_own_score_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(split.grid), block(TRACK_THREADS);
    for (int i = 0; i < n_rows; ++i) {
        a.e = row0 + i;
        a.row = curves_dev + rows_host[i].curve_off;
        a.weight = rows_host[i].weight;
        a.penalty = a.e == 0 ? 0.0 : penalty_host[i];
        a.reach = a.e == 0 ? 0 : reach_host[i];
        a.back = back_host[i];
        // (row 0 has no row before it: its launch's loads of D_in and P, which are always made and never used, go to its own
        // half -- keep: its own row -- and to P as it stands)
        a.D_in = D_dev + (keep ? (int64_t)(a.e == 0 ? 0 : a.e - 1) : (int64_t)((a.e + 1) & 1)) * n_shift;
        a.D_out = D_dev + (keep ? (int64_t)a.e : (int64_t)(a.e & 1)) * n_shift;
        a.move = move_dev + (int64_t)a.e * n_shift;
        a.from = from_dev + (int64_t)a.e * n_shift;
        const bool wide_step = wide_row(a.reach);
        if (wide_step) {
            launch_wide_tiles(a.D_in, n_shift, staged.tile_grid, w, st);
            if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
        }
        const int halo = wide_step ? 0 : track_halo_rounds(a.reach);
        const size_t tile_bytes = wide_step ? 0 : track_tile_bytes(split.per, a.reach);
        axis_dispatch(split.per, mx, [&](auto per, auto is_max) {
            if (wide_step) hipLaunchKernelGGL((wide_order_step_kernel<per.value, is_max.value>), grid, block, 0, st, a, w);
            else launch_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
            hipLaunchKernelGGL(order_scan_kernel<is_max.value>, dim3(1), block, 0, st, a);
            hipLaunchKernelGGL(order_apply_kernel<per.value>, grid, block, 0, st, a);
        });
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    return launch_ok();
}

// The margins walk, from the call's last row down.  wide: as track_forward_ordered's -- stage_order_margins' bound and workspace,
// and a row whose step into the row after it has a reach above TRACK_MAX_REACH goes through the tile pass (over C_{e+1}) and the
// wide step.
int track_order_margins(bool wide, const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                        const int32_t* back_host, const int32_t* guard_host, int n_rows, int32_t n_shift, int method,
                        const double* penalty_host, double step_cost, int row0, int n_total, const double* D_all_dev,
                        const int32_t* shift_dev, double* C_dev, double* S_dev, double* c_min_dev, double* through_dev, double* best_dev,
                        int32_t* best_arg_dev, double* alt_dev, int32_t* alt_arg_dev, double* M_dev, void* mem_dev, size_t mem_bytes,
                        void* hip_stream) {
    if (!curves_dev || !rows_host || !reach_host || !back_host || !guard_host || !penalty_host || !D_all_dev || !shift_dev || !C_dev ||
        !S_dev || !c_min_dev || !through_dev || !best_dev || !best_arg_dev || !alt_dev || !alt_arg_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    OrderMarginStage staged;
    const int rc = stage_order_margins(rows_host, reach_host, back_host, penalty_host, guard_host, n_rows, n_shift, n_curve, method,
                                       step_cost, row0, n_total, mem_dev, mem_bytes, staged, wide);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_all_dev | (uintptr_t)C_dev | (uintptr_t)S_dev | (uintptr_t)c_min_dev | (uintptr_t)through_dev | (uintptr_t)best_dev |
          (uintptr_t)alt_dev | (uintptr_t)M_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)shift_dev | (uintptr_t)best_arg_dev | (uintptr_t)alt_arg_dev) & 3))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    char* mem = (char*)mem_dev;
    const PathSplit& split = staged.split;
    const OrderMarginLayout& lay = staged.lay;
    const bool first_call = staged.first_call;
    const WideRecords w = wide_records(mem, staged.wide);
    OrderMarginArgs a;
    a.step_cost = step_cost;
    a.S = S_dev;
    a.shift = shift_dev;
    a.n_shift = n_shift;
    a.n_items = split.n_items;
    a.n_partials = (int)split.grid;
    a.in = margin_set(mem, lay.partials, 0);
    a.item_min = (double*)(mem + lay.item_min); a.item_arg = (int32_t*)(mem + lay.item_arg);
    a.after_min = (double*)(mem + lay.after_min);
    a.through = through_dev; a.best = best_dev; a.best_arg = best_arg_dev; a.alt = alt_dev; a.alt_arg = alt_arg_dev; a.c_min = c_min_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(split.grid), block(TRACK_THREADS);
    for (int i = n_rows - 1; i >= 0; --i) {
        a.e = row0 + i;
        a.last = a.e == n_total - 1;
        a.row = curves_dev + rows_host[i].curve_off;
        a.weight = rows_host[i].weight;
        a.reach = margin_reach_after(reach_host, i, n_rows, first_call);
        a.back = order_margin_back_after(back_host, i, n_rows, first_call);
        a.penalty = order_margin_penalty_after(penalty_host, i, n_rows, first_call);
        a.guard = guard_host[i];
        // (the sequence's last row has no row after it: its launch's loads of C_in and S, which are always made and never used, go
        // to the other half and to S as they stand)
        a.C_in = C_dev + (int64_t)((a.e + 1) & 1) * n_shift;
        a.C_out = C_dev + (int64_t)(a.e & 1) * n_shift;
        a.D_row = D_all_dev + (int64_t)a.e * n_shift;
        a.M_row = M_dev ? M_dev + (int64_t)a.e * n_shift : nullptr;
        const bool wide_step = wide_row(a.reach);
        if (wide_step) {
            launch_wide_tiles(a.C_in, n_shift, staged.tile_grid, w, st);
            if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
        }
        const int halo = wide_step ? 0 : track_halo_rounds(a.reach);
        const size_t tile_bytes = wide_step ? 0 : track_tile_bytes(split.per, a.reach);
        axis_dispatch(split.per, mx, [&](auto per, auto is_max) {
            if (wide_step) hipLaunchKernelGGL((wide_order_margin_step_kernel<per.value, is_max.value>), grid, block, 0, st, a, w);
            else launch_order_margin_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
            hipLaunchKernelGGL(order_margin_scan_kernel, dim3(1), block, 0, st, a);
            hipLaunchKernelGGL(order_margin_apply_kernel<per.value>, grid, block, 0, st, a);
        });
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    return launch_ok();
}
}  // namespace

extern "C" {

size_t sushi_hip_track_order_bytes(int n_rows, int32_t n_shift) { return order_layout_bytes(n_rows, n_shift); }
size_t sushi_hip_track_order_margins_bytes(int n_rows, int32_t n_shift) { return order_margin_layout_bytes(n_rows, n_shift); }
size_t sushi_hip_track_order_wide_bytes(int n_rows, int32_t n_shift) { return order_wide_layout_bytes(n_rows, n_shift); }
size_t sushi_hip_track_order_margins_wide_bytes(int n_rows, int32_t n_shift) { return order_margin_wide_layout_bytes(n_rows, n_shift); }

// the entry points: track_forward_ordered(keep, wide), track_order_margins(wide)
int sushi_hip_track_forward_ordered(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                    const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                    const double* penalty_host, double step_cost, int row0, int n_total, double* D_dev, int16_t* move_dev,
                                    double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                    int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward_ordered(false, false, curves_dev, n_curve, rows_host, reach_host, back_host, n_rows, n_shift, method, penalty_host,
                                     step_cost, row0, n_total, D_dev, move_dev, P_dev, from_dev, back_dev, row_min_dev, row_arg_dev,
                                     row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_forward_ordered_keep(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                         const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                         const double* penalty_host, double step_cost, int row0, int n_total, double* D_all_dev, int16_t* move_dev,
                                         double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                         int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward_ordered(true, false, curves_dev, n_curve, rows_host, reach_host, back_host, n_rows, n_shift, method, penalty_host,
                                     step_cost, row0, n_total, D_all_dev, move_dev, P_dev, from_dev, back_dev, row_min_dev, row_arg_dev,
                                     row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_forward_ordered_wide(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                         const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                         const double* penalty_host, double step_cost, int row0, int n_total, double* D_dev, int16_t* move_dev,
                                         double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                         int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward_ordered(false, true, curves_dev, n_curve, rows_host, reach_host, back_host, n_rows, n_shift, method, penalty_host,
                                     step_cost, row0, n_total, D_dev, move_dev, P_dev, from_dev, back_dev, row_min_dev, row_arg_dev,
                                     row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_forward_ordered_wide_keep(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                              const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                              const double* penalty_host, double step_cost, int row0, int n_total, double* D_all_dev, int16_t* move_dev,
                                              double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                              int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward_ordered(true, true, curves_dev, n_curve, rows_host, reach_host, back_host, n_rows, n_shift, method, penalty_host,
                                     step_cost, row0, n_total, D_all_dev, move_dev, P_dev, from_dev, back_dev, row_min_dev, row_arg_dev,
                                     row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_order_margins(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                  const int32_t* reach_host, const int32_t* back_host, const int32_t* guard_host, int n_rows,
                                  int32_t n_shift, int method, const double* penalty_host, double step_cost, int row0, int n_total,
                                  const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* S_dev, double* c_min_dev,
                                  double* through_dev, double* best_dev, int32_t* best_arg_dev, double* alt_dev, int32_t* alt_arg_dev,
                                  double* M_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_order_margins(false, curves_dev, n_curve, rows_host, reach_host, back_host, guard_host, n_rows, n_shift, method,
                                   penalty_host, step_cost, row0, n_total, D_all_dev, shift_dev, C_dev, S_dev, c_min_dev, through_dev,
                                   best_dev, best_arg_dev, alt_dev, alt_arg_dev, M_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_order_margins_wide(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                       const int32_t* reach_host, const int32_t* back_host, const int32_t* guard_host, int n_rows,
                                       int32_t n_shift, int method, const double* penalty_host, double step_cost, int row0, int n_total,
                                       const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* S_dev, double* c_min_dev,
                                       double* through_dev, double* best_dev, int32_t* best_arg_dev, double* alt_dev, int32_t* alt_arg_dev,
                                       double* M_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_order_margins(true, curves_dev, n_curve, rows_host, reach_host, back_host, guard_host, n_rows, n_shift, method,
                                   penalty_host, step_cost, row0, n_total, D_all_dev, shift_dev, C_dev, S_dev, c_min_dev, through_dev,
                                   best_dev, best_arg_dev, alt_dev, alt_arg_dev, M_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_backtrack_ordered(const int16_t* move_dev, const int32_t* from_dev, const int32_t* back_dev, const int32_t* row_arg_dev,
                                      int n_total, int32_t n_shift, int32_t* out_shift_dev, void* hip_stream) {
    return c_boundary([&]() -> int {
    if (!move_dev || !from_dev || !back_dev || !row_arg_dev || !out_shift_dev || n_total < 1 || n_shift < 1) return SUSHI_HIP_EINVAL;
    if (((uintptr_t)move_dev & 1) || (((uintptr_t)from_dev | (uintptr_t)back_dev | (uintptr_t)row_arg_dev | (uintptr_t)out_shift_dev) & 3))
        return SUSHI_HIP_EALIGN;
    hipLaunchKernelGGL(order_backtrack_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, move_dev, from_dev, back_dev, row_arg_dev,
                       n_total, n_shift, out_shift_dev);
    return launch_ok();
}); }

}  // extern "C"
