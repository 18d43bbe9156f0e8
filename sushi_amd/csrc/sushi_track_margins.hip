// sushi_amd/csrc/sushi_track_margins.hip -- sushi_hip_track_margins: the min-marginals of the tracking pass (gfx950).
//
// M_e[j] is the cost of the best whole path that puts event e at shift j: the forward pass's D_e[j] (kept by
// sushi_hip_track_forward_keep) plus B_e[j], what the events after e add.  B comes from the same recurrence run from the last row
// down: C_e[j] = u_e[j] + B_e[j], B_e[j] = min(min_{|d| <= reach_{e+1}} (C_{e+1}[j + d] + step_cost |d|), n_{e+1} + penalty), in the
// arithmetic include/sushi_hip.h states and track_core.hpp / track_margin_core.hpp implement (float64, products and sums rounded
// separately: this unit is compiled with -ffp-contract=off).  The output is bit-identical to the NumPy restatement
// (sushi_amd/track.py track_margins_host).
//
// The shape is sushi_track.hip's: one plain launch per row, stream-ordered, from the call's last row down; C lives in two halves
// (row e reads half (e + 1) & 1 and writes half e & 1); thread t of a work item holds the shift indices t, t + 256, ...; a work
// item stages its PER x 256 values of C_{e+1} and reach_{e+1} values on each side once into LDS and reads every candidate but its
// own from there, in the order -1, +1, -2, +2, ....  Beside that a thread reads D_e[j], forms M and C, and the workgroup leaves one
// partial record of three first minima -- of C, of M, and of M outside the guard window around s_e (the backtrack's output: read
// from device memory, workgroup-uniform) -- which the next launch reduces before anything else; the thread that owns s_e stores
// through_e.  No grid waits on itself, and there are no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "track_margin_core.hpp"
#include "path_device.hpp"
#include "track_margin_device.hpp"

namespace {

using namespace sushi;

#include "sushi_track_margins_step.inc"     // MarginArgs, margin_step_kernel, margin_close_kernel, launch_margin_step

}  // namespace

extern "C" {

size_t sushi_hip_track_margins_bytes(int n_rows, int32_t n_shift) { return margin_layout_bytes(n_rows, n_shift); }

int sushi_hip_track_margins(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                            const int32_t* guard_host, int n_rows, int32_t n_shift, int method, double penalty, double step_cost,
                            int row0, int n_total, const double* D_all_dev, const int32_t* shift_dev, double* C_dev, double* c_min_dev,
                            double* through_dev, double* best_dev, int32_t* best_arg_dev, double* alt_dev, int32_t* alt_arg_dev,
                            double* M_dev, void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
    if (!curves_dev || !rows_host || !reach_host || !guard_host || !D_all_dev || !shift_dev || !C_dev || !c_min_dev || !through_dev ||
        !best_dev || !best_arg_dev || !alt_dev || !alt_arg_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    MarginStage staged;
    const int rc = stage_margins(rows_host, reach_host, guard_host, n_rows, n_shift, n_curve, method, penalty, step_cost, row0, n_total,
                                 mem_dev, mem_bytes, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_all_dev | (uintptr_t)C_dev | (uintptr_t)c_min_dev | (uintptr_t)through_dev | (uintptr_t)best_dev |
          (uintptr_t)alt_dev | (uintptr_t)M_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)shift_dev | (uintptr_t)best_arg_dev | (uintptr_t)alt_arg_dev) & 3))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    MarginArgs a;
    a.penalty = penalty;
    a.step_cost = step_cost;
    a.shift = shift_dev;
    a.n_shift = n_shift;
    a.n_items = staged.split.n_items;
    a.n_partials = (int)staged.split.grid;
    a.through = through_dev; a.best = best_dev; a.best_arg = best_arg_dev; a.alt = alt_dev; a.alt_arg = alt_arg_dev; a.c_min = c_min_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(staged.split.grid), block(TRACK_THREADS);
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
        const int halo = track_halo_rounds(a.reach);
        const size_t tile_bytes = track_tile_bytes(staged.split.per, a.reach);
        axis_dispatch(staged.split.per, mx, [&](auto per, auto is_max) {
            launch_margin_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
        });
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    a.e = row0;
    a.in = margin_set((char*)mem_dev, staged.lay, (n_rows - 1) & 1);
    hipLaunchKernelGGL(margin_close_kernel, dim3(1), block, 0, st, a);
    return launch_ok();
}); }

}  // extern "C"
