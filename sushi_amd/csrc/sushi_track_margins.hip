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

struct MarginArgs {
    const float* row;                       // R_e: curves + curve_off
    double weight, penalty, step_cost;
    const double* C_in;                     // [n_shift] C_{e+1}: half (e + 1) & 1
    double* C_out;                          // [n_shift] C_e: half e & 1
    const double* D_row;                    // [n_shift] D_e
    double* M_row;                          // [n_shift] M_e, or null
    const int32_t* shift;                   // [n_total] s_e
    int32_t n_shift;
    int32_t reach;                          // reach_{e+1} (0 for the sequence's last row)
    int32_t guard;                          // guard_e
    int64_t n_items;
    int e;                                  // the row of the sequence
    int prev;                               // where n_{e+1} comes from (path_device.hpp PREV_*; PREV_ROW_MIN: c_min[e + 1])
    int n_partials;                         // records of `in`
    MarginPartials in, out;
    double* through; double* best; int32_t* best_arg; double* alt; int32_t* alt_arg; double* c_min;    // the whole sequence's
};

// HALO: the rounds of 256 halo values a launch loads (track_halo_rounds(reach): 0 at reach 0, where nothing is staged)
template <int PER, bool MAX, int HALO>
__global__ __launch_bounds__(TRACK_THREADS)
void margin_step_kernel(MarginArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    constexpr int SPAN = PER * TRACK_THREADS;
    __shared__ PathLds lds;
    extern __shared__ double tile[];        // [reach + SPAN + reach]: entry l is C_{e+1}[item's first index - reach + l]
    const float* __restrict__ row = a.row;
    const double* __restrict__ Cin = a.C_in;
    const double* __restrict__ Drow = a.D_row;
    double* __restrict__ Cout = a.C_out;
    double* __restrict__ Mrow = a.M_row;
    const int32_t n_shift = a.n_shift;
    const int32_t reach = HALO == 0 ? 0 : a.reach;
    const bool last = a.prev == PREV_NONE;  // the sequence's last row: there is no B
    const int32_t s_e = path_clamp(a.shift[a.e], n_shift);
    const int32_t guard = a.guard;
    double jump = 0.0;
    if (a.prev == PREV_PARTIALS) jump = reduce_margin_partials(a, blockIdx.x == 0, a.e + 1, lds) + a.penalty;
    else if (a.prev == PREV_ROW_MIN) jump = a.c_min[a.e + 1] + a.penalty;

    MinD best_c = {INFINITY, PATH_NO_INDEX}, best_m = {INFINITY, PATH_NO_INDEX}, best_a = {INFINITY, PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        // (an item's first index is below n_shift < 2^31; the indices behind it may pass 2^31 only where they are not used: 64 bits)
        const int64_t base = item * SPAN;
        const int64_t j0 = base + threadIdx.x;
        // every load is always made, the indices outside the axis moved onto an element inside it (axis_at): the tile, the halo,
        // the row and D_e are all asked for before the first value is used
        int32_t at[PER];
        float r[PER];
        double c[PER], dd[PER];
        double hv[HALO > 0 ? HALO : 1];
        int32_t hl[HALO > 0 ? HALO : 1];    // where a halo value goes in the tile; -1: this thread has none in that round
#pragma unroll
        for (int p = 0; p < PER; ++p) at[p] = axis_at(j0 + p * TRACK_THREADS, n_shift);
#pragma unroll
        for (int p = 0; p < PER; ++p) c[p] = Cin[at[p]];
        if (HALO > 0) {
#pragma unroll
            for (int k = 0; k < HALO; ++k) {
                // halo entry h of 2 * reach: the left side's h < reach at index base - reach + h, the right side's at base + SPAN + h - reach
                const int32_t h = (int32_t)threadIdx.x + k * TRACK_THREADS;
                const bool left = h < reach;
                int64_t g = left ? base - reach + h : base + SPAN + (h - reach);
                g = g < 0 ? 0 : g;
                hl[k] = h < 2 * reach ? (left ? h : SPAN + h) : -1;
                hv[k] = Cin[axis_at(g, n_shift)];
            }
        }
#pragma unroll
        for (int p = 0; p < PER; ++p) dd[p] = Drow[at[p]];
#pragma unroll
        for (int p = 0; p < PER; ++p) r[p] = row[at[p]];
        // (nothing is scheduled across this line: the loads above are all in flight before the first is waited for)
        __builtin_amdgcn_sched_barrier(0);
        if (HALO > 0) {
            __syncthreads();                // the readers of the item before this one are through
#pragma unroll
            for (int p = 0; p < PER; ++p) tile[reach + (int32_t)threadIdx.x + p * TRACK_THREADS] = c[p];
#pragma unroll
            for (int k = 0; k < HALO; ++k)
                if (hl[k] >= 0) tile[hl[k]] = hv[k];
            __syncthreads();
        }
        // nearB[j]: the thread's own value is cand(0); the others come from the tile in the order -1, +1, -2, +2, ..., in which
        // track_replaces is the strict comparison (the value only: no move word).  room: how far index j may move down / up inside
        // the axis and the reach
        double near[PER];
        int32_t room_lo[PER], room_hi[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS, up = (int64_t)n_shift - 1 - j;
            near[p] = c[p];
            room_lo[p] = (int32_t)(j < reach ? j : reach);
            room_hi[p] = (int32_t)(up < 0 ? -1 : (up < reach ? up : reach));
        }
        if (HALO > 0) {
            for (int32_t s = 1; s <= reach; ++s) {
                const double price = track_price(a.step_cost, s);
#pragma unroll
                for (int p = 0; p < PER; ++p) {
                    const int32_t l = reach + (int32_t)threadIdx.x + p * TRACK_THREADS;
                    const double lo = track_cand(tile[l - s], price), hi = track_cand(tile[l + s], price);
                    // (selects: a candidate outside the axis was loaded from an element inside it, and is left out here)
                    const bool take_lo = (int)(s <= room_lo[p]) & (int)track_replaces_in_order(lo, near[p]);
                    near[p] = take_lo ? lo : near[p];
                    const bool take_hi = (int)(s <= room_hi[p]) & (int)track_replaces_in_order(hi, near[p]);
                    near[p] = take_hi ? hi : near[p];
                }
            }
        }
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * TRACK_THREADS;
            const bool valid = j < n_shift;
            const double u = path_cost(METHOD, a.weight, r[p]);
            const double b = margin_back(near[p], jump);
            const double m = margin_through(dd[p], b, last);
            const double cn = margin_suffix(u, b, last);
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

// closes a call's last launch (row row0): one workgroup turns its partial records into the row's outputs
__global__ __launch_bounds__(TRACK_THREADS)
void margin_close_kernel(MarginArgs a) {
    __shared__ PathLds lds;
    reduce_margin_partials(a, true, a.e, lds);
}

template <int PER, bool MAX>
void launch_margin_step(int halo, dim3 grid, size_t tile_bytes, hipStream_t st, const MarginArgs& a) {
    const dim3 block(TRACK_THREADS);
    if (halo == 0) hipLaunchKernelGGL((margin_step_kernel<PER, MAX, 0>), grid, block, 0, st, a);
    else if (halo == TRACK_HALO_SMALL) hipLaunchKernelGGL((margin_step_kernel<PER, MAX, TRACK_HALO_SMALL>), grid, block, tile_bytes, st, a);
    else hipLaunchKernelGGL((margin_step_kernel<PER, MAX, TRACK_HALO_LARGE>), grid, block, tile_bytes, st, a);
}

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
