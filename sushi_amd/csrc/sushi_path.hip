// sushi_amd/csrc/sushi_path.hip -- sushi_hip_path_forward / sushi_hip_path_backtrack: where the shift a sequence of score rows shares
// changes (gfx950).
//
// The rows of a sequence (sushi_hip_match_curves output, each from a curve_off of its own) lie on one shift axis in event order.  The
// pass chooses a shift per row that minimises the sum of the weighted costs plus `penalty` for every change of shift between
// consecutive rows: D_e[j] = u_e[j] + min(D_{e-1}[j], m_{e-1} + penalty), in the arithmetic include/sushi_hip.h states and
// path_core.hpp implements (float64, product and sum rounded separately: this unit is compiled with -ffp-contract=off).  The output
// is bit-identical to the NumPy restatement (sushi_amd/segments.py path_host).
//
// One plain launch per row, stream-ordered: the launch boundary is the pass's only all-to-all (m_{e-1}), and no grid waits on
// itself.  Thread t of a work item holds the shift indices t, t + 256, ...: lane <-> consecutive index, so a wave's load of the row is
// one contiguous span wherever the row starts, its 64 stay decisions are one ballot, and D is updated in place.  The minimum of D_e
// has no 64-bit key (a float64 and an index), so every workgroup leaves one partial record, and every workgroup of the next launch
// begins by reducing those records under a rule that does not depend on the order they meet in (the lower index wins a tie):
// path_device.hpp, which the tracking pass (sushi_track.hip) shares.  A row's curve_off and weight are arguments of its launch:
// nothing is uploaded.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "path_core.hpp"
#include "path_device.hpp"

namespace {

using namespace sushi;

struct PathArgs {
    const float* row;                       // R_e: curves + curve_off
    double weight, penalty;
    double* D;                              // [n_shift] in: D_{e-1}, out: D_e
    unsigned long long* stay;               // [words] row e's stay bits
    int32_t n_shift;
    int64_t n_items;
    int e;                                  // the row of the sequence
    int prev;                               // where m_{e-1} comes from: PREV_NONE (e = 0: there is none), PREV_PARTIALS (`in`, which the
                                            // launch before this one left), PREV_ROW_MIN (row_min[e - 1]: an earlier call's last row)
    int n_partials;                         // records of `in`
    PathPartials in, out;
    double* row_min; int32_t* row_arg; int32_t* row_own_index; float* row_own_score;    // the whole sequence's
};

template <int PER, bool MAX>
__global__ __launch_bounds__(PATH_THREADS)
void path_step_kernel(PathArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    __shared__ PathLds lds;
    const float* __restrict__ row = a.row;
    double* D = a.D;
    const int32_t n_shift = a.n_shift;
    const bool first = a.prev == PREV_NONE;
    double jump = 0.0;
    if (a.prev == PREV_PARTIALS) jump = reduce_partials<METHOD>(a.in, a.n_partials, blockIdx.x == 0, a.e - 1, a, lds) + a.penalty;
    else if (a.prev == PREV_ROW_MIN) jump = a.row_min[a.e - 1] + a.penalty;

    MinD best = {INFINITY, PATH_NO_INDEX};
    OwnF own = {own_worst<METHOD>(), PATH_NO_INDEX};
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        // (an item's first index is below n_shift < 2^31; the indices behind it may pass 2^31 only where they are not used: 64 bits)
        const int64_t j0 = item * (PER * PATH_THREADS) + threadIdx.x;
        // every load is always made, the indices past the end moved onto the last element (axis_at): a load under a branch would
        // make the wait counts assume the worst
        int32_t at[PER];
        float r[PER];
        double d[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) at[p] = axis_at(j0 + p * PATH_THREADS, n_shift);
#pragma unroll
        for (int p = 0; p < PER; ++p) r[p] = row[at[p]];
#pragma unroll
        for (int p = 0; p < PER; ++p) d[p] = D[at[p]];
        // (nothing is scheduled across this line: without it the PER = 2 kernel consumed its first pair before it asked for the second)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            const int64_t j = j0 + p * PATH_THREADS;
            const bool valid = j < n_shift;
            const double u = path_cost(METHOD, a.weight, r[p]);
            bool st = false;
            const double stepped = path_step(d[p], u, jump, &st);
            const double dn = first ? u : stepped;
            // a wave's lanes hold 64 consecutive indices from a multiple of 64 on: one word of the row's bits, tail bits zero
            const unsigned long long bits = __ballot((int)valid & (int)!first & (int)st);
            // (selects, not branches: a value used only under `valid` has its load moved into the branch, behind a full wait)
            const bool take = (int)valid & (int)path_min_replaces(dn, (int32_t)j, best.v, best.i);
            best.v = take ? dn : best.v; best.i = take ? (int32_t)j : best.i;
            const bool take_own = (int)valid & (int)path_own_replaces(METHOD, r[p], (int32_t)j, own.v, own.i);
            own.v = take_own ? r[p] : own.v; own.i = take_own ? (int32_t)j : own.i;
            if (valid) {
                D[j] = dn;
                if ((threadIdx.x & 63) == 0) a.stay[j >> 6] = bits;
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

// closes a call's last row: one workgroup turns its partial records into the row's outputs
template <bool MAX>
__global__ __launch_bounds__(PATH_THREADS)
void path_close_kernel(PathArgs a) {
    constexpr int METHOD = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    __shared__ PathLds lds;
    reduce_partials<METHOD>(a.in, a.n_partials, true, a.e, a, lds);
}

// one wave; lane 0 walks the rows backwards: every step reads the bit the step before it chose
__global__ __launch_bounds__(64)
void path_backtrack_kernel(const unsigned long long* stay, const int32_t* row_arg, int n_total, int32_t n_shift, int32_t* out_shift) {
    if (threadIdx.x == 0 && blockIdx.x == 0) path_backtrack((const uint64_t*)stay, row_arg, n_total, n_shift, out_shift);
}

}  // namespace

extern "C" {

size_t sushi_hip_path_bytes(int n_rows, int32_t n_shift) { return path_layout_bytes(n_rows, n_shift); }

int64_t sushi_hip_path_stay_words(int32_t n_shift) { return path_stay_words(n_shift); }

int sushi_hip_path_forward(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, int n_rows, int32_t n_shift,
                           int method, double penalty, int row0, int n_total, double* D_dev, unsigned long long* stay_dev,
                           double* row_min_dev, int32_t* row_arg_dev, int32_t* row_own_index_dev, float* row_own_score_dev,
                           void* mem_dev, size_t mem_bytes, void* hip_stream) { return c_boundary([&]() -> int {
    if (!curves_dev || !rows_host || !D_dev || !stay_dev || !row_min_dev || !row_arg_dev || !row_own_index_dev || !row_own_score_dev ||
        !mem_dev) return SUSHI_HIP_EINVAL;
    PathStage staged;
    const int rc = stage_path(rows_host, n_rows, n_shift, n_curve, method, penalty, row0, n_total, mem_dev, mem_bytes, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if ((((uintptr_t)D_dev | (uintptr_t)stay_dev | (uintptr_t)row_min_dev) & 7) ||
        (((uintptr_t)curves_dev | (uintptr_t)row_arg_dev | (uintptr_t)row_own_index_dev | (uintptr_t)row_own_score_dev) & 3))
        return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    PathArgs a;
    a.penalty = penalty;
    a.D = D_dev;
    a.n_shift = n_shift;
    a.n_items = staged.split.n_items;
    a.n_partials = (int)staged.split.grid;
    a.row_min = row_min_dev; a.row_arg = row_arg_dev; a.row_own_index = row_own_index_dev; a.row_own_score = row_own_score_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(staged.split.grid), block(PATH_THREADS);
    for (int i = 0; i < n_rows; ++i) {
        a.e = row0 + i;
        a.row = curves_dev + rows_host[i].curve_off;
        a.weight = rows_host[i].weight;
        a.stay = stay_dev + (int64_t)a.e * staged.words;
        a.prev = a.e == 0 ? PREV_NONE : (i == 0 ? PREV_ROW_MIN : PREV_PARTIALS);
        a.in = partial_set((char*)mem_dev, staged.lay, (i + 1) & 1);
        a.out = partial_set((char*)mem_dev, staged.lay, i & 1);
        axis_dispatch(staged.split.per, mx, [&](auto per, auto is_max) {
            hipLaunchKernelGGL((path_step_kernel<per.value, is_max.value>), grid, block, 0, st, a);
        });
        if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    }
    a.e = row0 + n_rows - 1;
    a.in = partial_set((char*)mem_dev, staged.lay, (n_rows - 1) & 1);
    if (mx) hipLaunchKernelGGL(path_close_kernel<true>, dim3(1), block, 0, st, a);
    else hipLaunchKernelGGL(path_close_kernel<false>, dim3(1), block, 0, st, a);
    return launch_ok();
}); }

int sushi_hip_path_backtrack(const unsigned long long* stay_dev, const int32_t* row_arg_dev, int n_total, int32_t n_shift,
                             int32_t* out_shift_dev, void* hip_stream) { return c_boundary([&]() -> int {
    if (!stay_dev || !row_arg_dev || !out_shift_dev || n_total < 1 || n_shift < 1) return SUSHI_HIP_EINVAL;
    if (((uintptr_t)stay_dev & 7) || (((uintptr_t)row_arg_dev | (uintptr_t)out_shift_dev) & 3)) return SUSHI_HIP_EALIGN;
    hipLaunchKernelGGL(path_backtrack_kernel, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, stay_dev, row_arg_dev, n_total, n_shift,
                       out_shift_dev);
    return launch_ok();
}); }

}  // extern "C"
