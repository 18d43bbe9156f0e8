// sushi_amd/csrc/sushi_track_order_margins.hip -- sushi_hip_track_order_margins: the min-marginals of the ordered tracking pass
// (gfx950).
//
// M_e[j] = D_e[j] + B_e[j], D the ordered forward pass's rows (kept by sushi_hip_track_forward_ordered_keep) and B what the events
// after e add: B_e[j] = min(nearB[j], S_{e+1}[t'_e(j)] + penalty_{e+1}), nearB the window minimum over C_{e+1}, S_{e+1} the suffix
// minimum of C_{e+1} and t'_e(j) = max(j - back_{e+1}, 0); C_e[j] = u_e[j] + B_e[j] -- the arithmetic include/sushi_hip.h "ordered
// margins" states and track_margin_core.hpp / track_order_margin_core.hpp implement (float64, -ffp-contract=off).  The output is
// bit-identical to the NumPy restatement (sushi_amd/track.py track_ordered_margins_host); with every back unlimited and one penalty
// it is sushi_track_margins.hip's, bit for bit.
//
// Three plain launches per row, from the call's last row down, stream-ordered; the launch boundary is the only synchronisation,
// and no workgroup waits on another:
//   step   sushi_track_margins.hip's step kernel -- the window minimum over an LDS tile of C_{e+1}, the <PER, MAX, HALO> dispatch,
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
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "track_order_margin_core.hpp"
#include "path_device.hpp"
#include "track_margin_device.hpp"

namespace {

using namespace sushi;

#include "sushi_track_order_margins_step.inc"   // OrderMarginArgs, order_margin_step_kernel, _scan_kernel, _apply_kernel, the launcher

}  // namespace

extern "C" {

size_t sushi_hip_track_order_margins_bytes(int n_rows, int32_t n_shift) { return order_margin_layout_bytes(n_rows, n_shift); }

int sushi_hip_track_order_margins(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, const int32_t* reach_host,
                                  const int32_t* back_host, const int32_t* guard_host, int n_rows, int32_t n_shift, int method,
                                  const double* penalty_host, double step_cost, int row0, int n_total, const double* D_all_dev,
                                  const int32_t* shift_dev, double* C_dev, double* S_dev, double* c_min_dev, double* through_dev,
                                  double* best_dev, int32_t* best_arg_dev, double* alt_dev, int32_t* alt_arg_dev, double* M_dev,
                                  void* mem_dev, size_t mem_bytes, void* hip_stream) {
    return c_boundary([&]() -> int {
    if (!curves_dev || !rows_host || !reach_host || !back_host || !guard_host || !penalty_host || !D_all_dev || !shift_dev || !C_dev ||
        !S_dev || !c_min_dev || !through_dev || !best_dev || !best_arg_dev || !alt_dev || !alt_arg_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    OrderMarginStage staged;
    const int rc = stage_order_margins(rows_host, reach_host, back_host, penalty_host, guard_host, n_rows, n_shift, n_curve, method,
                                       step_cost, row0, n_total, mem_dev, mem_bytes, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_all_dev | (uintptr_t)C_dev | (uintptr_t)S_dev | (uintptr_t)c_min_dev | (uintptr_t)through_dev | (uintptr_t)best_dev |
          (uintptr_t)alt_dev | (uintptr_t)M_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)shift_dev | (uintptr_t)best_arg_dev | (uintptr_t)alt_arg_dev) & 3))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    char* mem = (char*)mem_dev;
    OrderMarginArgs a;
    a.step_cost = step_cost;
    a.S = S_dev;
    a.shift = shift_dev;
    a.n_shift = n_shift;
    a.n_items = staged.split.n_items;
    a.n_partials = (int)staged.split.grid;
    a.in = margin_set(mem, staged.lay.partials, 0);
    a.item_min = (double*)(mem + staged.lay.item_min); a.item_arg = (int32_t*)(mem + staged.lay.item_arg);
    a.after_min = (double*)(mem + staged.lay.after_min);
    a.through = through_dev; a.best = best_dev; a.best_arg = best_arg_dev; a.alt = alt_dev; a.alt_arg = alt_arg_dev; a.c_min = c_min_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(staged.split.grid), block(TRACK_THREADS);
    for (int i = n_rows - 1; i >= 0; --i) {
        a.e = row0 + i;
        a.last = a.e == n_total - 1;
        a.row = curves_dev + rows_host[i].curve_off;
        a.weight = rows_host[i].weight;
        a.reach = margin_reach_after(reach_host, i, n_rows, staged.first_call);
        a.back = order_margin_back_after(back_host, i, n_rows, staged.first_call);
        a.penalty = order_margin_penalty_after(penalty_host, i, n_rows, staged.first_call);
        a.guard = guard_host[i];
        // (the sequence's last row has no row after it: its launch's loads of C_in and S, which are always made and never used, go
        // to the other half and to S as they stand)
        a.C_in = C_dev + (int64_t)((a.e + 1) & 1) * n_shift;
        a.C_out = C_dev + (int64_t)(a.e & 1) * n_shift;
        a.D_row = D_all_dev + (int64_t)a.e * n_shift;
        a.M_row = M_dev ? M_dev + (int64_t)a.e * n_shift : nullptr;
        const int halo = track_halo_rounds(a.reach);
        const size_t tile_bytes = track_tile_bytes(staged.split.per, a.reach);
        axis_dispatch(staged.split.per, mx, [&](auto per, auto is_max) {
            launch_order_margin_step<per.value, is_max.value>(halo, grid, tile_bytes, st, a);
            hipLaunchKernelGGL(order_margin_scan_kernel, dim3(1), block, 0, st, a);
            hipLaunchKernelGGL(order_margin_apply_kernel<per.value>, grid, block, 0, st, a);
        });
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    return launch_ok();
}); }

}  // extern "C"
