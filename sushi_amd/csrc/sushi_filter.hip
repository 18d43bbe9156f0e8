// sushi_amd/csrc/sushi_filter.hip -- sushi_hip_filter: a row through a FIR filter of float64 taps (gfx950).
//
// Output i is the sum over k = 0 .. T - 1, in that order, of taps[k] * (x[clamp(in_start + i + k - a)] - centre), a = (T - 1) / 2,
// in the arithmetic include/sushi_hip.h states and filter_core.hpp implements (float64; the product and the sum round separately:
// this unit is compiled with -ffp-contract=off), so that the output is bit-identical to the NumPy restatement
// (sushi_amd/filter.py filter_host).
//
// A workgroup of 256 threads owns a tile of consecutive outputs (filter_tile(T): 2048 up to 1025 taps, 1024 above) and strides
// over the tiles on a fixed grid.  Its LDS is sized by the call (filter_lds_bytes(T): 23 KB at 255 taps, 47 KB at 2047, never more
// than 48 KB), and the grid is as many workgroups as the CUs hold of that size, five a CU at the most.  The taps come into LDS
// once per workgroup.  Per tile:
//   1. the tile's tile + T - 1 deviations come into LDS as float64, both clamps applied here (sample by sample: consecutive lanes
//      read consecutive samples; in_start has only sample alignment).  Element e lies in slot e + e / PER.
//   2. a thread forms PER consecutive outputs with PER accumulators.  It holds a window of 2 PER - 1 staged samples in registers;
//      a block of PER taps costs it PER sample reads and PER tap reads (one address for the whole wave) for PER * PER products
//      and as many additions.  Each accumulator walks k upwards, so the PER addition chains hide each other's latency.
//   3. it finishes and stores its outputs (out_dev has only sample alignment: plain stores).
// No atomics, no workspace, no workgroup waits on another.  Bound by float64 issue, not by LDS reads (profiles/filter/README.md).
// SUSHI_FILTER_STRIDED (an A/B build only, tools/filter_rates.py): a thread owns outputs 256 apart instead -- unpadded slots, no
// conflicts and no reuse: PER sample reads per tap.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "filter_core.hpp"

namespace {

using namespace sushi;

struct FilterArgs {
    const void* in;
    int64_t n_in, in_start;
    const double* taps;
    int32_t n_taps, tile;
    int64_t n_tiles;
    void* out;
    int64_t out_len;
};

template <class T, int PER>
__global__ __launch_bounds__(FILTER_THREADS)
void filter_kernel(FilterArgs a) {
    extern __shared__ __align__(16) double filter_lds[];     // filter_lds_bytes(T): the taps, then the staged samples
    const T* __restrict__ x = (const T*)a.in;
    T* __restrict__ out = (T*)a.out;
    const int32_t n_taps = a.n_taps;
    double* __restrict__ taps = filter_lds;
    double* __restrict__ stage = filter_lds + n_taps + 1;
    const int32_t n_stage = FILTER_THREADS * PER + n_taps - 1;       // the whole tile's samples, also for a short last tile
    const int tid = threadIdx.x;
    for (int32_t k = tid; k < n_taps; k += FILTER_THREADS) taps[k] = a.taps[k];
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t i0 = tile * (int64_t)(FILTER_THREADS * PER);
        const int32_t n_out = (int32_t)(a.out_len - i0 < FILTER_THREADS * PER ? a.out_len - i0 : FILTER_THREADS * PER);
        const int64_t g0 = a.in_start + i0 - filter_lead(n_taps);    // the tile's first sample (may lie outside the row)
        // 1. stage, four samples a thread in flight
        for (int32_t e0 = tid; e0 < n_stage; e0 += 4 * FILTER_THREADS) {
            T v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + u * FILTER_THREADS < n_stage) v[u] = row_at(x, a.n_in, g0 + e0 + u * FILTER_THREADS);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t e = e0 + u * FILTER_THREADS;
#ifdef SUSHI_FILTER_STRIDED
                if (e < n_stage) stage[e] = filter_deviation(v[u]);
#else
                if (e < n_stage) stage[filter_slot(e, PER)] = filter_deviation(v[u]);
#endif
            }
        }
        __syncthreads();
        // 2. the sums
        double acc[PER];
#pragma unroll
        for (int r = 0; r < PER; ++r) acc[r] = 0.0;
#ifdef SUSHI_FILTER_STRIDED
        {
            const double* __restrict__ s = stage + tid;
            int32_t k = 0;
            for (; k + 4 <= n_taps; k += 4) {
                double h[4], w[4][PER];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    h[j] = taps[k + j];
#pragma unroll
                    for (int r = 0; r < PER; ++r) w[j][r] = s[k + j + r * FILTER_THREADS];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < PER; ++r) acc[r] = filter_step(acc[r], h[j], w[j][r]);
            }
            for (; k < n_taps; ++k) {
                const double h = taps[k];
#pragma unroll
                for (int r = 0; r < PER; ++r) acc[r] = filter_step(acc[r], h, s[k + r * FILTER_THREADS]);
            }
        }
#pragma unroll
        for (int r = 0; r < PER; ++r)
            if (tid + r * FILTER_THREADS < n_out) out[i0 + tid + r * FILTER_THREADS] = filter_finish(acc[r], (const T*)0);
#else
        {
            // element tid * PER + c lies in slot tid * (PER + 1) + c + c / PER; w[q] holds element tid * PER + kb + q
            const double* __restrict__ s = stage + tid * (PER + 1);
            double w[2 * PER - 1];
#pragma unroll
            for (int q = 0; q < PER - 1; ++q) w[q] = s[q];
            int32_t kb = 0;
            for (; kb + PER <= n_taps; kb += PER) {
                const double* __restrict__ sb = s + kb + kb / PER;      // c = kb + q: kb is a multiple of PER
                double h[PER];
#pragma unroll
                for (int q = PER - 1; q < 2 * PER - 1; ++q) w[q] = sb[q + q / PER];
#pragma unroll
                for (int j = 0; j < PER; ++j) h[j] = taps[kb + j];
#pragma unroll
                for (int j = 0; j < PER; ++j)
#pragma unroll
                    for (int r = 0; r < PER; ++r) acc[r] = filter_step(acc[r], h[j], w[j + r]);
#pragma unroll
                for (int q = 0; q < PER - 1; ++q) w[q] = w[q + PER];
            }
            const int32_t rest = n_taps - kb;                           // < PER taps left: the same block, tap by tap
            const double* __restrict__ sb = s + kb + kb / PER;
#pragma unroll
            for (int j = 0; j < PER - 1; ++j) {
                if (j < rest) {                                          // (the same for the whole workgroup)
                    const double h = taps[kb + j];
                    w[PER - 1 + j] = sb[PER - 1 + j + (PER - 1 + j) / PER];
#pragma unroll
                    for (int r = 0; r < PER; ++r) acc[r] = filter_step(acc[r], h, w[j + r]);
                }
            }
        }
        // 3. outputs
#pragma unroll
        for (int r = 0; r < PER; ++r)
            if (tid * PER + r < n_out) out[i0 + tid * PER + r] = filter_finish(acc[r], (const T*)0);
#endif
        __syncthreads();                                    // the next tile stages over what this one read
    }
}

template <class T>
void launch(const FilterArgs& a, const FilterStage& s, hipStream_t st) {
    if (filter_per_thread(a.n_taps) == FILTER_WIDE)
        hipLaunchKernelGGL((filter_kernel<T, FILTER_WIDE>), dim3(s.grid), dim3(FILTER_THREADS), s.lds_bytes, st, a);
    else
        hipLaunchKernelGGL((filter_kernel<T, FILTER_NARROW>), dim3(s.grid), dim3(FILTER_THREADS), s.lds_bytes, st, a);
}

}  // namespace

extern "C" {

int sushi_hip_filter(const void* in_dev, int dtype, int64_t n_in, int64_t in_start, const double* taps_dev, int32_t n_taps,
                     void* out_dev, int64_t out_len, void* hip_stream) { return c_boundary([&]() -> int {
    FilterStage staged;
    const int rc = stage_filter(in_dev, dtype, n_in, in_start, taps_dev, n_taps, out_dev, out_len, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if (!row_aligned(in_dev, dtype) || !row_aligned(out_dev, dtype) || ((uintptr_t)taps_dev & 7)) return SUSHI_HIP_EALIGN;

    FilterArgs a;
    a.in = in_dev; a.n_in = n_in; a.in_start = in_start; a.taps = taps_dev; a.n_taps = n_taps; a.tile = staged.tile;
    a.n_tiles = staged.n_tiles; a.out = out_dev; a.out_len = out_len;
    row_dispatch(dtype, [&](auto t) { launch<decltype(t)>(a, staged, (hipStream_t)hip_stream); });
    return launch_ok();
}); }

}  // extern "C"
