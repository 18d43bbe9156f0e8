// sushi_amd/csrc/sushi_joint.hip -- sushi_hip_joint_reduce: the one shift a group of score rows shares (gfx950).
//
// A group's rows (sushi_hip_match_curves output, each from a curve_off of its own) are put on one joint axis, summed by weight in
// row order in the arithmetic include/sushi_hip.h states and joint_core.hpp implements (float64, product and sum rounded separately:
// this unit is compiled with -ffp-contract=off), and reduced to the first extremum of the sum -- and, in the same pass, to every
// row's own first extremum.  The output is bit-identical to the NumPy restatement (sushi_amd/joint.py joint_host).
//
// One launch serves all groups: a group's joint indices are cut into work items of PER * 256 consecutive ones, a workgroup finds its
// item's group by bisection of the items' running count.  Thread t of an item holds the indices t, t + 256, ...: lane <-> consecutive
// index, so a wave's load of one row is one contiguous 256-byte span wherever the row starts, and every byte of every row is read
// once (a group's last item reads its row's last float again for the indices past the end).  The rows are taken ROWS_AHEAD at a time: their loads are all issued before the first is consumed, the sums stay in row
// order.  Extrema leave a wave as 64-bit (score, index) keys through atomicMin (sushi_common.hpp), so the result does not depend on
// scheduling.  A second small launch turns the keys into the outputs and gathers every row's score at the joint answer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "joint_core.hpp"
#include "axis_device.hpp"         // how an extremum leaves a wave: joint_key, wave_key_min, thread_key

namespace {

using namespace sushi;

constexpr int ROWS_AHEAD = 4;       // rows whose loads are in flight together (x PER loads each)

struct JointArgs {
    const float* curves;
    const JointGroupDev* groups;
    const JointRowDev* rows;
    unsigned long long* group_keys;
    unsigned long long* row_keys;
    int n_groups, n_rows;
    int64_t n_items;
    float* out_joint;               // or NULL
    int32_t* out_idx; float* out_score;
    float* out_row_score; int32_t* out_row_idx; float* out_row_best;
};

template <int PER, bool MAX>
__global__ __launch_bounds__(AXIS_THREADS)
void joint_reduce_kernel(JointArgs a) {
    const float* __restrict__ curves = a.curves;
    const JointRowDev* __restrict__ rows = a.rows;
    for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        int lo = 0, hi = a.n_groups - 1;                    // the last group whose first item is not behind `item`
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.groups[mid].first_item <= item) lo = mid; else hi = mid - 1;
        }
        const JointGroupDev g = a.groups[lo];
        const int32_t n_shift = g.n_shift;
        // (an item's first index is below n_shift < 2^31; the indices behind it may pass 2^31 only where they are not used: 64 bits)
        const int64_t j0 = (item - g.first_item) * (PER * AXIS_THREADS) + threadIdx.x;
        // where the thread's loads go: its indices, those past the group's end moved onto the last one (axis_at)
        int32_t at[PER];
        double acc[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) {
            at[p] = axis_at(j0 + p * AXIS_THREADS, n_shift);
            acc[p] = 0.0;
        }
        int i = 0;
        for (; i + ROWS_AHEAD <= g.n_rows; i += ROWS_AHEAD) {
            float v[ROWS_AHEAD][PER];
            double w[ROWS_AHEAD];
            int64_t off[ROWS_AHEAD];
#pragma unroll
            for (int u = 0; u < ROWS_AHEAD; ++u) {          // (the rows' records first: a record read between two rows' loads would wait for the loads)
                off[u] = rows[g.first_row + i + u].curve_off;
                w[u] = rows[g.first_row + i + u].weight;
            }
#pragma unroll
            for (int u = 0; u < ROWS_AHEAD; ++u) {
                const float* __restrict__ x = curves + off[u];
#pragma unroll
                for (int p = 0; p < PER; ++p) v[u][p] = x[at[p]];
            }
#pragma unroll
            for (int u = 0; u < ROWS_AHEAD; ++u) {
#pragma unroll
                for (int p = 0; p < PER; ++p) acc[p] = joint_accumulate(acc[p], w[u], v[u][p]);
                wave_key_min(thread_key<PER, MAX>(v[u], j0, n_shift), a.row_keys + g.first_row + i + u);
            }
        }
        for (; i < g.n_rows; ++i) {
            const JointRowDev r = rows[g.first_row + i];
            const float* __restrict__ x = curves + r.curve_off;
            float v[PER];
#pragma unroll
            for (int p = 0; p < PER; ++p) v[p] = x[at[p]];
#pragma unroll
            for (int p = 0; p < PER; ++p) acc[p] = joint_accumulate(acc[p], r.weight, v[p]);
            wave_key_min(thread_key<PER, MAX>(v, j0, n_shift), a.row_keys + g.first_row + i);
        }
        float joint[PER];
#pragma unroll
        for (int p = 0; p < PER; ++p) joint[p] = (float)acc[p];
        if (a.out_joint) {
            float* __restrict__ o = a.out_joint + g.joint_off + j0;
#pragma unroll
            for (int p = 0; p < PER; ++p)
                if (j0 + p * AXIS_THREADS < n_shift) o[p * AXIS_THREADS] = joint[p];
        }
        wave_key_min(thread_key<PER, MAX>(joint, j0, n_shift), a.group_keys + lo);
    }
}

// Keys -> outputs.  Thread t < n_groups: group t's index and the joint value there (formed again: joint_value); thread t < n_rows:
// row t's own first extremum and its score at its group's joint index.  The values are read where they lie, not taken from the keys
// (a key holds -0.0 as 0.0).  An index a key could not hold (a NaN row: unspecified results) is taken as 0: no access leaves the rows.
__global__ __launch_bounds__(AXIS_THREADS)
void joint_gather_kernel(JointArgs a) {
    const int t = blockIdx.x * AXIS_THREADS + threadIdx.x;
    if (t < a.n_groups) {
        const JointGroupDev g = a.groups[t];
        uint32_t idx = key_pos(a.group_keys[t]);
        if (idx >= (uint32_t)g.n_shift) idx = 0;
        a.out_idx[t] = (int32_t)idx;
        a.out_score[t] = joint_value(a.curves, a.rows, g.first_row, g.n_rows, (int64_t)idx);
    }
    if (t < a.n_rows) {
        const JointRowDev r = a.rows[t];
        const int32_t n_shift = a.groups[r.group].n_shift;
        uint32_t idx = key_pos(a.group_keys[r.group]);
        if (idx >= (uint32_t)n_shift) idx = 0;
        uint32_t own = key_pos(a.row_keys[t]);
        if (own >= (uint32_t)n_shift) own = 0;
        a.out_row_score[t] = a.curves[r.curve_off + idx];
        a.out_row_idx[t] = (int32_t)own;
        a.out_row_best[t] = a.curves[r.curve_off + own];
    }
}

}  // namespace

extern "C" {

size_t sushi_hip_joint_bytes(int n_groups, int n_rows) { return joint_layout_bytes(n_groups, n_rows); }

int sushi_hip_joint_reduce(const float* curves_dev, int64_t n_curve, const SushiHipJointRow* rows_host, int n_rows,
                           const SushiHipJointGroup* groups_host, int n_groups, int method, void* mem_dev, size_t mem_bytes,
                           int32_t* out_idx_dev, float* out_score_dev, float* out_row_score_dev, int32_t* out_row_idx_dev,
                           float* out_row_best_dev, float* out_joint_dev, void* hip_stream) { return c_boundary([&]() -> int {
    if (!curves_dev || !rows_host || !groups_host || !mem_dev || !out_idx_dev || !out_score_dev || !out_row_score_dev ||
        !out_row_idx_dev || !out_row_best_dev) return SUSHI_HIP_EINVAL;
    JointStage staged;
    const int rc = stage_joint(rows_host, n_rows, groups_host, n_groups, n_curve, method, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if (((uintptr_t)mem_dev & 255) || (((uintptr_t)curves_dev | (uintptr_t)out_idx_dev | (uintptr_t)out_score_dev |
         (uintptr_t)out_row_score_dev | (uintptr_t)out_row_idx_dev | (uintptr_t)out_row_best_dev | (uintptr_t)out_joint_dev) & 3))
        return SUSHI_HIP_EALIGN;
    if (mem_bytes < staged.lay.bytes) return SUSHI_HIP_ENOSPACE;

    hipStream_t st = (hipStream_t)hip_stream;
    // (The source is pageable host memory that dies with this call.  ASSUMED: the runtime has taken its copy of such a source when
    // hipMemcpyAsync returns.)
    if (hipMemcpyAsync(mem_dev, staged.image.data(), staged.image.size(), hipMemcpyHostToDevice, st) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    char* mem = (char*)mem_dev;
    JointArgs a;
    a.curves = curves_dev;
    a.groups = (const JointGroupDev*)(mem + staged.lay.groups);
    a.rows = (const JointRowDev*)(mem + staged.lay.rows);
    a.group_keys = (unsigned long long*)(mem + staged.lay.group_keys);
    a.row_keys = (unsigned long long*)(mem + staged.lay.row_keys);
    a.n_groups = n_groups; a.n_rows = n_rows; a.n_items = staged.n_items;
    a.out_joint = out_joint_dev;
    a.out_idx = out_idx_dev; a.out_score = out_score_dev;
    a.out_row_score = out_row_score_dev; a.out_row_idx = out_row_idx_dev; a.out_row_best = out_row_best_dev;
    const dim3 grid(staged.grid), block(AXIS_THREADS);
    axis_dispatch(staged.per, method == SUSHI_HIP_METHOD_CCOEFF_NORMED, [&](auto per, auto mx) {
        hipLaunchKernelGGL((joint_reduce_kernel<per.value, mx.value>), grid, block, 0, st, a);
    });
    if (hipGetLastError() != hipSuccess) return SUSHI_HIP_ELAUNCH;
    hipLaunchKernelGGL(joint_gather_kernel, dim3((unsigned)((n_rows + AXIS_THREADS - 1) / AXIS_THREADS)), block, 0, st, a);
    return launch_ok();
}); }

}  // extern "C"
