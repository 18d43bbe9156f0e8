// sushi_amd/csrc/sushi_track.hip -- sushi_hip_track_forward / sushi_hip_track_backtrack: a shift that wanders from event to event
// (gfx950); and sushi_hip_track_forward_keep, the same launches with every row of D kept (for sushi_track_margins.hip).
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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "track_core.hpp"
#include "path_device.hpp"

namespace {

using namespace sushi;

#include "sushi_track_step.inc"             // TrackArgs, track_step_kernel, track_close_kernel, launch_step

// one wave; lane 0 walks the rows backwards: every step reads the move the step before it chose
__global__ __launch_bounds__(64)
void track_backtrack_kernel(const int16_t* move, const int32_t* row_arg, int n_total, int32_t n_shift, int32_t* out_shift) {
    if (threadIdx.x == 0 && blockIdx.x == 0) track_backtrack(move, row_arg, n_total, n_shift, out_shift);
}

}  // namespace

extern "C" {

size_t sushi_hip_track_bytes(int n_rows, int32_t n_shift) { return track_layout_bytes(n_rows, n_shift); }

// sushi_hip_track_forward and sushi_hip_track_forward_keep: one body.  keep: D_dev holds every row ([n_total][n_shift]: row e reads
// row e - 1 and writes row e) instead of two halves used by turns; the launches, and so the bits, are the same.
static int track_forward(bool keep, const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host,
                         const int32_t* reach_host, int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0,
                         int n_total, double* D_dev, int16_t* move_dev, double* row_min_dev, int32_t* row_arg_dev,
                         int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    if (!curves_dev || !rows_host || !reach_host || !D_dev || !move_dev || !row_min_dev || !row_arg_dev || !row_own_index_dev ||
        !row_own_score_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    TrackStage staged;
    const int rc = stage_track(rows_host, reach_host, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total, mem_dev,
                               mem_bytes, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_dev | (uintptr_t)row_min_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)row_arg_dev | (uintptr_t)row_own_index_dev | (uintptr_t)row_own_score_dev) & 3) ||
        ((uintptr_t)move_dev & 1))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    TrackArgs a;
    a.penalty = penalty;
    a.step_cost = step_cost;
    a.n_shift = n_shift;
    a.n_items = staged.split.n_items;
    a.n_partials = (int)staged.split.grid;
    a.row_min = row_min_dev; a.row_arg = row_arg_dev; a.row_own_index = row_own_index_dev; a.row_own_score = row_own_score_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(staged.split.grid), block(TRACK_THREADS);
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
        const int halo = track_halo_rounds(a.reach);
        const size_t tile_bytes = track_tile_bytes(staged.split.per, a.reach);
        axis_dispatch(staged.split.per, mx, [&](auto per, auto is_max) {
            launch_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
        });
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    a.e = row0 + n_rows - 1;
    a.in = partial_set((char*)mem_dev, staged.lay, (n_rows - 1) & 1);
    if (mx) hipLaunchKernelGGL(track_close_kernel<true>, dim3(1), block, 0, st, a);
    else hipLaunchKernelGGL(track_close_kernel<false>, dim3(1), block, 0, st, a);
    return launch_ok();
}

int sushi_hip_track_forward(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                            int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0, int n_total,
                            double* D_dev, int16_t* move_dev, double* row_min_dev, int32_t* row_arg_dev, int32_t* row_own_index_dev,
                            float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward(false, curves_dev, n_curve, rows_host, reach_host, n_rows, n_shift, method, penalty, step_cost, row0, n_total,
                             D_dev, move_dev, row_min_dev, row_arg_dev, row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
}); }

int sushi_hip_track_forward_keep(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                 int n_rows, int32_t n_shift, int method, double penalty, double step_cost, int row0, int n_total,
                                 double* D_all_dev, int16_t* move_dev, double* row_min_dev, int32_t* row_arg_dev,
                                 int32_t* row_own_index_dev, float* row_own_score_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
        return track_forward(true, curves_dev, n_curve, rows_host, reach_host, n_rows, n_shift, method, penalty, step_cost, row0, n_total,
                             D_all_dev, move_dev, row_min_dev, row_arg_dev, row_own_index_dev, row_own_score_dev, mem_dev, mem_bytes, hip_stream);
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
