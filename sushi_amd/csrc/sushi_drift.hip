// sushi_amd/csrc/sushi_drift.hip -- sushi_hip_drift_reduce: score rows summed along sloped lines of shifts (gfx950).
//
// The rows of E events (sushi_hip_match_curves output, each from a curve_off of its own) lie on one shift axis.  A candidate d is one
// int32 offset per row; its line is line[d][j] = sum_e w_e * R_e[j + o[d][e]] in the arithmetic include/sushi_hip.h states and
// drift_core.hpp implements (joint_accumulate unchanged: float64, product and sum rounded separately -- this unit is compiled with
// -ffp-contract=off), taken over the j for which every row is addressed inside itself.  The answer is the first extremum over all
// (candidate, j) in table order.  The output is bit-identical to the NumPy restatement (sushi_amd/drift.py drift_host).
//
// A work item is PER * 256 consecutive j times DRIFT_DB consecutive candidates; one grid strides over the items.  Thread t of an item
// holds the indices t, t + 256, ... for each of the DRIFT_DB candidates: lane <-> consecutive j, so every load of a wave is one
// contiguous 256-byte span, and the DRIFT_DB spans of one row lie a few floats apart -- the vector cache serves them from the lines the
// first of them fetched, a row's bytes come from L2 once per item and block.  A load whose j + o leaves the row (j outside the
// candidate's range, or past the axis's end) is moved onto an index inside it and its value is not used: no branch around a load.  The
// rows are taken ROWS_AHEAD at a time, their loads all issued before the first is consumed, the sums stay in row order.  Extrema leave
// a wave as 64-bit (score, j) keys through atomicMin into one slot per candidate; a second launch turns them into the per-candidate
// outputs and sends (score_d, d) keys into one slot; a third reads the answer and gathers every row's score there.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "drift_core.hpp"
#include "axis_device.hpp"         // how an extremum leaves a wave: joint_key, wave_key_min

namespace {

using namespace sushi;

constexpr int DB = DRIFT_DB;
// rows whose loads are in flight together (x DB x PER loads each): about 64 loads, at most four rows
constexpr int rows_ahead(int per) { return 64 / (DB * per) < 1 ? 1 : 64 / (DB * per) > 4 ? 4 : 64 / (DB * per); }

struct DriftArgs {
    const float* curves;
    const SushiHipJointRow* rows;
    const int32_t* offs;                // [blocks][n_rows][DB]
    const DriftRange* ranges;           // [blocks * DB]
    unsigned long long* keys;           // [blocks * DB]
    unsigned long long* best_key;
    int n_rows, n_drifts;
    int32_t n_shift;
    int64_t n_jitems, n_items;
    float* out_lines;                   // or NULL
    int32_t* out_best; float* out_score;
    float* out_row_score;
    int32_t* out_drift_idx; float* out_drift_score;
};

// Where the load of index `at` (inside the row) under offset o goes.  at + o lies in (-n_shift, 2 * n_shift - 1): taken modulo 2^32
// it is below n_shift exactly when it is inside the row (n_shift < 2^31), else the load stays at `at`.
__device__ __forceinline__ uint32_t drift_at(uint32_t at, int32_t o, uint32_t n_shift) {
    const uint32_t t = at + (uint32_t)o;
    return t < n_shift ? t : at;
}

template <int PER, bool MAX>
__global__ __launch_bounds__(AXIS_THREADS)
void drift_reduce_kernel(DriftArgs a) {
    constexpr int RA = rows_ahead(PER);
    constexpr int method = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    const float* __restrict__ curves = a.curves;
    const SushiHipJointRow* __restrict__ rows = a.rows;
    const int32_t n_shift = a.n_shift;
    const int n_rows = a.n_rows;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int64_t blk = item / a.n_jitems;
        // (an item's first index is below n_shift < 2^31; the indices behind it may pass 2^31 only where they are not used: 64 bits)
        const int64_t j0 = (item - blk * a.n_jitems) * (PER * AXIS_THREADS) + threadIdx.x;
        const int32_t* __restrict__ ob = a.offs + blk * n_rows * DB;
        uint32_t at[PER];
        double acc[DB][PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            at[p] = (uint32_t)axis_at(j0 + p * AXIS_THREADS, n_shift);
#pragma unroll
            for (int u = 0; u < DB; ++u) acc[u][p] = 0.0;
        }
        int e = 0;
        for (; e + RA <= n_rows; e += RA) {
            float v[RA][DB][PER];
            double w[RA];
            int64_t off[RA];
            int32_t o[RA][DB];
#pragma unroll
            for (int r = 0; r < RA; ++r) {                  // (the rows' records and offsets first: one read between two rows' loads would wait for the loads)
                off[r] = rows[e + r].curve_off;
                w[r] = rows[e + r].weight;
#pragma unroll
                for (int u = 0; u < DB; ++u) o[r][u] = ob[(int64_t)(e + r) * DB + u];
            }
            __builtin_amdgcn_sched_barrier(0);              // (the scheduler would sink a record's read between two rows' loads)
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const float* __restrict__ x = curves + off[r];
#pragma unroll
                for (int u = 0; u < DB; ++u)
#pragma unroll
                    for (int p = 0; p < PER; ++p) v[r][u][p] = x[drift_at(at[p], o[r][u], (uint32_t)n_shift)];
            }
#pragma unroll
            for (int r = 0; r < RA; ++r)
#pragma unroll
                for (int u = 0; u < DB; ++u)
#pragma unroll
                    for (int p = 0; p < PER; ++p) acc[u][p] = joint_accumulate(acc[u][p], w[r], v[r][u][p]);
        }
        for (; e < n_rows; ++e) {
            const SushiHipJointRow r = rows[e];
            const float* __restrict__ x = curves + r.curve_off;
            int32_t o[DB];
            float v[DB][PER];
#pragma unroll
            for (int u = 0; u < DB; ++u) o[u] = ob[(int64_t)e * DB + u];
#pragma unroll
            for (int u = 0; u < DB; ++u)
#pragma unroll
                for (int p = 0; p < PER; ++p) v[u][p] = x[drift_at(at[p], o[u], (uint32_t)n_shift)];
#pragma unroll
            for (int u = 0; u < DB; ++u)
#pragma unroll
                for (int p = 0; p < PER; ++p) acc[u][p] = joint_accumulate(acc[u][p], r.weight, v[u][p]);
        }
        // a candidate's values on its valid range -> its line, and the thread's first extremum of them as a key
#pragma unroll
        for (int u = 0; u < DB; ++u) {
            const int64_t d = blk * DB + u;
            const DriftRange range = a.ranges[d];           // (the last block's padding: an empty range, no store, no key)
            float* __restrict__ line = a.out_lines && d < a.n_drifts ? a.out_lines + d * n_shift : nullptr;
            bool have = false;
            float best = 0.0f;
            int64_t where = 0;
#pragma unroll
            for (int p = 0; p < PER; ++p) {
                const int64_t j = j0 + p * AXIS_THREADS;
                const bool valid = j >= range.lo && j < range.hi;
                const float s = (float)acc[u][p];
                if (line && j < n_shift) line[j] = valid ? s : (MAX ? -INFINITY : INFINITY);
                if (valid && (!have || axis_better(method, s, best))) { best = s; where = j; have = true; }
            }
            wave_key_min(have ? joint_key<MAX>(best, (unsigned)where) : NO_KEY, a.keys + d);
        }
    }
}

// Keys -> the per-candidate outputs.  Thread t < n_drifts: candidate t's index and its line's value there (formed again: drift_value),
// and the key (score_t, t) into the answer's slot: the smallest is the best score at its first candidate in table order.  An index a
// key could not hold (a NaN row: unspecified results) is taken as the range's first: no access leaves the rows.
template <bool MAX>
__global__ __launch_bounds__(AXIS_THREADS)
void drift_candidates_kernel(DriftArgs a) {
    const int t = blockIdx.x * AXIS_THREADS + threadIdx.x;
    unsigned long long key = NO_KEY;
    if (t < a.n_drifts) {
        const DriftRange range = a.ranges[t];
        uint32_t idx = key_pos(a.keys[t]);
        if (idx < (uint32_t)range.lo || idx >= (uint32_t)range.hi) idx = (uint32_t)range.lo;
        const float score = drift_value(a.curves, a.rows, a.n_rows, a.offs, t, (int64_t)idx);
        a.out_drift_idx[t] = (int32_t)idx;
        a.out_drift_score[t] = score;
        key = joint_key<MAX>(score, (unsigned)t);
    }
    wave_key_min(key, a.best_key);
}

// The answer, and every row's own score there, read where it lies (a key holds -0.0 as 0.0).
__global__ __launch_bounds__(AXIS_THREADS)
void drift_gather_kernel(DriftArgs a) {
    const int t = blockIdx.x * AXIS_THREADS + threadIdx.x;
    uint32_t d = key_pos(*a.best_key);
    if (d >= (uint32_t)a.n_drifts) d = 0;
    const int32_t j = a.out_drift_idx[d];
    if (t == 0) {
        a.out_best[0] = (int32_t)d;
        a.out_best[1] = j;
        a.out_score[0] = a.out_drift_score[d];
    }
    if (t < a.n_rows) a.out_row_score[t] = a.curves[a.rows[t].curve_off + j + a.offs[drift_offset_at(a.n_rows, (int)d, t)]];
}

}  // namespace

extern "C" {

size_t sushi_hip_drift_bytes(int n_rows, int n_drifts) { return drift_layout_bytes(n_rows, n_drifts); }

int sushi_hip_drift_reduce(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, int n_rows, int32_t n_shift,
                           const int32_t* offsets_host, int n_drifts, int method, void* mem_dev, size_t mem_bytes,
                           int32_t* out_best_dev, float* out_score_dev, float* out_row_score_dev, int32_t* out_drift_idx_dev,
                           float* out_drift_score_dev, float* out_lines_dev, void* hip_stream) { return c_boundary([&]() -> int {
    if (!curves_dev || !mem_dev || !out_best_dev || !out_score_dev || !out_row_score_dev || !out_drift_idx_dev ||
        !out_drift_score_dev) return SUSHI_HIP_EINVAL;
    DriftStage staged;
    const int rc = stage_drift(rows_host, n_rows, n_shift, offsets_host, n_drifts, n_curve, method, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if (((uintptr_t)mem_dev & 255) || (((uintptr_t)curves_dev | (uintptr_t)out_best_dev | (uintptr_t)out_score_dev |
         (uintptr_t)out_row_score_dev | (uintptr_t)out_drift_idx_dev | (uintptr_t)out_drift_score_dev | (uintptr_t)out_lines_dev) & 3))
        return SUSHI_HIP_EALIGN;
    if (mem_bytes < staged.lay.bytes) return SUSHI_HIP_ENOSPACE;

    hipStream_t st = (hipStream_t)hip_stream;
    // (The source is pageable host memory that dies with this call.  ASSUMED: the runtime has taken its copy of such a source when
    // hipMemcpyAsync returns.)
    if (hipMemcpyAsync(mem_dev, staged.image.data(), staged.image.size(), hipMemcpyHostToDevice, st) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    char* mem = (char*)mem_dev;
    DriftArgs a;
    a.curves = curves_dev;
    a.rows = (const SushiHipJointRow*)(mem + staged.lay.rows);
    a.offs = (const int32_t*)(mem + staged.lay.offs);
    a.ranges = (const DriftRange*)(mem + staged.lay.ranges);
    a.keys = (unsigned long long*)(mem + staged.lay.keys);
    a.best_key = (unsigned long long*)(mem + staged.lay.best_key);
    a.n_rows = n_rows; a.n_drifts = n_drifts; a.n_shift = n_shift;
    a.n_jitems = staged.n_jitems; a.n_items = staged.n_items;
    a.out_lines = out_lines_dev;
    a.out_best = out_best_dev; a.out_score = out_score_dev; a.out_row_score = out_row_score_dev;
    a.out_drift_idx = out_drift_idx_dev; a.out_drift_score = out_drift_score_dev;
    const bool mx = method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const dim3 grid(staged.grid), block(AXIS_THREADS);
    axis_dispatch(staged.per, mx, [&](auto per, auto is_max) {
        hipLaunchKernelGGL((drift_reduce_kernel<per.value, is_max.value>), grid, block, 0, st, a);
    });
    if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    const dim3 by_drift((unsigned)((n_drifts + AXIS_THREADS - 1) / AXIS_THREADS));
    if (mx) hipLaunchKernelGGL(drift_candidates_kernel<true>, by_drift, block, 0, st, a);
    else hipLaunchKernelGGL(drift_candidates_kernel<false>, by_drift, block, 0, st, a);
    if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    hipLaunchKernelGGL(drift_gather_kernel, dim3((unsigned)((n_rows + AXIS_THREADS - 1) / AXIS_THREADS)), block, 0, st, a);
    return launch_ok();
}); }

}  // extern "C"
