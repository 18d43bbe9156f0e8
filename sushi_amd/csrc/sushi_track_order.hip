// sushi_amd/csrc/sushi_track_order.hip -- sushi_hip_track_forward_ordered / sushi_hip_track_backtrack_ordered: the tracking pass
// (sushi_track.hip) with events kept in order -- a jump into (e, j) comes from an index of row e - 1 no further than back_e above j,
// at a penalty of row e's own (gfx950).
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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "track_order_core.hpp"
#include "path_device.hpp"

namespace {

using namespace sushi;

#include "sushi_track_order_step.inc"       // OrderArgs, order_step_kernel, order_scan_kernel, order_apply_kernel, launch_step

// one wave; lane 0 walks the rows backwards: every step reads the move the step before it chose
__global__ __launch_bounds__(64)
void order_backtrack_kernel(const int16_t* move, const int32_t* from, const int32_t* back, const int32_t* row_arg, int n_total,
                            int32_t n_shift, int32_t* out_shift) {
    if (threadIdx.x == 0 && blockIdx.x == 0) order_backtrack(move, from, back, row_arg, n_total, n_shift, out_shift);
}

}  // namespace

extern "C" {

size_t sushi_hip_track_order_bytes(int n_rows, int32_t n_shift) { return order_layout_bytes(n_rows, n_shift); }

// sushi_hip_track_forward_ordered and sushi_hip_track_forward_ordered_keep: one body.  keep: D_dev holds every row ([n_total][n_shift]:
// row e reads row e - 1 and writes row e) instead of two halves used by turns; the launches, and so the bits, are the same.
static int track_forward_ordered(bool keep, const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                 const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                 const double* penalty_host, double step_cost, int row0, int n_total, double* D_dev, int16_t* move_dev,
                                 double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                 int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes,
                                 void* hip_stream) {
    if (!curves_dev || !rows_host || !reach_host || !back_host || !penalty_host || !D_dev || !move_dev || !P_dev || !from_dev ||
        !back_dev || !row_min_dev || !row_arg_dev || !row_own_index_dev || !row_own_score_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    OrderStage staged;
    const int rc = stage_track_ordered(rows_host, reach_host, back_host, penalty_host, n_rows, n_shift, n_curve, method, step_cost, row0,
                                       n_total, mem_dev, mem_bytes, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_dev | (uintptr_t)P_dev | (uintptr_t)row_min_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)from_dev | (uintptr_t)back_dev | (uintptr_t)row_arg_dev | (uintptr_t)row_own_index_dev |
          (uintptr_t)row_own_score_dev) & 3) ||
        ((uintptr_t)move_dev & 1))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    char* mem = (char*)mem_dev;
    OrderArgs a;
    a.step_cost = step_cost;
    a.P = P_dev;
    a.back_dev = back_dev;
    a.n_shift = n_shift;
    a.n_items = staged.split.n_items;
    a.n_partials = (int)staged.split.grid;
    a.partials = partial_set(mem, staged.lay.partials, 0);
    a.item_min = (double*)(mem + staged.lay.item_min); a.item_arg = (int32_t*)(mem + staged.lay.item_arg);
    a.before_min = (double*)(mem + staged.lay.before_min); a.before_arg = (int32_t*)(mem + staged.lay.before_arg);
    a.row_min = row_min_dev; a.row_arg = row_arg_dev; a.row_own_index = row_own_index_dev; a.row_own_score = row_own_score_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(staged.split.grid), block(TRACK_THREADS);
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
        const int halo = track_halo_rounds(a.reach);
        const size_t tile_bytes = track_tile_bytes(staged.split.per, a.reach);
        axis_dispatch(staged.split.per, mx, [&](auto per, auto is_max) {
            launch_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
            hipLaunchKernelGGL(order_scan_kernel<is_max.value>, dim3(1), block, 0, st, a);
            hipLaunchKernelGGL(order_apply_kernel<per.value>, grid, block, 0, st, a);
        });
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    return launch_ok();
}

int sushi_hip_track_forward_ordered(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                    const int32_t* back_host, int n_rows, int32_t n_shift, int method, const double* penalty_host,
                                    double step_cost, int row0, int n_total, double* D_dev, int16_t* move_dev, double* P_dev,
                                    int32_t* from_dev, int32_t* back_dev, double* row_min_dev, int32_t* row_arg_dev,
                                    int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes,
                                    void* hip_stream) { return c_boundary([&]() -> int {
    return track_forward_ordered(false, curves_dev, n_curve, rows_host, reach_host, back_host, n_rows, n_shift, method, penalty_host,
                                 step_cost, row0, n_total, D_dev, move_dev, P_dev, from_dev, back_dev, row_min_dev, row_arg_dev,
                                 row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_forward_ordered_keep(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                                         const int32_t* reach_host, const int32_t* back_host, int n_rows, int32_t n_shift, int method,
                                         const double* penalty_host, double step_cost, int row0, int n_total, double* D_all_dev,
                                         int16_t* move_dev, double* P_dev, int32_t* from_dev, int32_t* back_dev, double* row_min_dev,
                                         int32_t* row_arg_dev, int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev,
                                         size_t mem_bytes, void* hip_stream) { return c_boundary([&]() -> int {
    return track_forward_ordered(true, curves_dev, n_curve, rows_host, reach_host, back_host, n_rows, n_shift, method, penalty_host,
                                 step_cost, row0, n_total, D_all_dev, move_dev, P_dev, from_dev, back_dev, row_min_dev, row_arg_dev,
                                 row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
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
