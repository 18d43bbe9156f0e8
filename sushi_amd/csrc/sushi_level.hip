// sushi_amd/csrc/sushi_level.hip -- sushi_hip_level: a row divided by its local level (gfx950).
//
// Output i is q = (d_g * W) / ((E + fw) * peak) held to [-1, 1] and put back on the sample type's scale, with d_g the deviation of
// sample g = in_start + i from the type's centre and E the sum of |d| over the W samples around it, in the arithmetic
// include/sushi_hip.h states and level_core.hpp implements (this unit is compiled with -ffp-contract=off), so that the output is
// bit-identical to the NumPy restatement (sushi_amd/level.py level_host).
//
// A workgroup of 256 threads owns a tile of consecutive outputs and strides over the tiles on a fixed grid, four workgroups a CU
// at the most.  No atomics, no workspace, no workgroup waits on another.  in_dev and out_dev have only sample alignment: samples
// are read and stored one by one, consecutive lanes at consecutive samples.
//
// float32 (level_f32_kernel) -- the window sum is float64 and sequential in t, so it is filter_kernel without taps.  Per tile of
// 2048 outputs:
//   1. the tile's 2048 + W - 1 signed deviations come into LDS as float64, both clamps applied here; element e lies in slot
//      e + e / 8 (level_f32_lds_bytes(W): 18 KB at W = 1, 27 KB at 1023).
//   2. a thread forms 8 consecutive outputs with 8 accumulators, each walking t upwards.  It holds a window of 15 staged values in
//      registers: a block of 8 steps costs it 8 LDS reads for 64 additions of |w| (the absolute value is an operand modifier).
//      A sliding update would change the bits.
//   3. d_g is the staged value at t = h; the thread finishes and stores its outputs.
//
// uint8 (level_u8_kernel) -- the window sum is an exact integer, so it comes from a prefix sum, at a cost that does not grow with
// W.  Per tile of 4096 outputs:
//   1. the tile's 4096 + W - 1 bytes come into LDS, both clamps applied here.
//   2. a thread sums |d| over its 21 consecutive bytes; a wave scan of the threads' totals (shuffles) and the four waves' totals
//      in LDS give its base; it writes P[k], the sum over the tile's first k bytes, for its 21 places (an odd stride in words:
//      the lanes of a store meet different banks).
//   3. a thread finishes 16 outputs 256 apart: E = P[i + W] - P[i], d_g from the staged byte at i + h, the quotient in float64.
//      Consecutive lanes read consecutive words and store consecutive bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "level_core.hpp"

namespace {

using namespace sushi;

struct LevelArgs {
    const void* in;
    int64_t n_in, in_start;
    int32_t window;
    int64_t n_tiles;
    double fw, peak;          // level_floor_term(floor, W); peak
    void* out;
    int64_t out_len;
};

__global__ __launch_bounds__(LEVEL_THREADS)
void level_f32_kernel(LevelArgs a) {
    constexpr int PER = LEVEL_F32_PER;
    extern __shared__ __align__(16) double level_stage[];      // level_f32_lds_bytes(W): the staged deviations
    const float* __restrict__ x = (const float*)a.in;
    float* __restrict__ out = (float*)a.out;
    const int32_t window = a.window, lead = level_lead(window);
    const int32_t n_stage = LEVEL_F32_TILE + window - 1;        // the whole tile's samples, also for a short last tile
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t i0 = tile * (int64_t)LEVEL_F32_TILE;
        const int32_t n_out = (int32_t)(a.out_len - i0 < LEVEL_F32_TILE ? a.out_len - i0 : LEVEL_F32_TILE);
        const int64_t g0 = a.in_start + i0 - lead;               // the tile's first sample (may lie outside the row)
        // 1. stage, four samples a thread in flight
        for (int32_t e0 = tid; e0 < n_stage; e0 += 4 * LEVEL_THREADS) {
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + u * LEVEL_THREADS < n_stage) v[u] = row_at(x, a.n_in, g0 + e0 + u * LEVEL_THREADS);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t e = e0 + u * LEVEL_THREADS;
                if (e < n_stage) level_stage[level_f32_slot(e)] = row_deviation(v[u]);
            }
        }
        __syncthreads();
        // 2. the window sums: element tid * PER + c lies in slot tid * (PER + 1) + c + c / PER; w[q] holds element tid * PER + tb + q
        const double* __restrict__ s = level_stage + tid * (PER + 1);
        double acc[PER], w[2 * PER - 1];
#pragma unroll
        for (int r = 0; r < PER; ++r) acc[r] = 0.0;
#pragma unroll
        for (int q = 0; q < PER - 1; ++q) w[q] = s[q];
        int32_t tb = 0;
        for (; tb + PER <= window; tb += PER) {
            const double* __restrict__ sb = s + tb + tb / PER;      // c = tb + q: tb is a multiple of PER
#pragma unroll
            for (int q = PER - 1; q < 2 * PER - 1; ++q) w[q] = sb[q + q / PER];
#pragma unroll
            for (int j = 0; j < PER; ++j)
#pragma unroll
                for (int r = 0; r < PER; ++r) acc[r] = acc[r] + level_abs(w[j + r]);
#pragma unroll
            for (int q = 0; q < PER - 1; ++q) w[q] = w[q + PER];
        }
        {
            const int32_t rest = window - tb;                        // < PER steps left: the same block, step by step
            const double* __restrict__ sb = s + tb + tb / PER;
#pragma unroll
            for (int j = 0; j < PER - 1; ++j) {
                if (j < rest) {                                      // (the same for the whole workgroup)
                    w[PER - 1 + j] = sb[PER - 1 + j + (PER - 1 + j) / PER];
#pragma unroll
                    for (int r = 0; r < PER; ++r) acc[r] = acc[r] + level_abs(w[j + r]);
                }
            }
        }
        // 3. outputs: d_g is element tid * PER + r + h
#pragma unroll
        for (int r = 0; r < PER; ++r) {
            const int32_t c = r + lead;
            if (tid * PER + r < n_out) out[i0 + tid * PER + r] = level_output<float>(s[c + c / PER], acc[r], window, a.fw, a.peak);
        }
        __syncthreads();                                    // the next tile stages over what this one read
    }
}

__global__ __launch_bounds__(LEVEL_THREADS)
void level_u8_kernel(LevelArgs a) {
    extern __shared__ __align__(16) uint32_t level_words[];    // LEVEL_U8_LDS_BYTES: P, the waves' totals, the staged bytes
    uint32_t* __restrict__ prefix = level_words;
    uint32_t* __restrict__ wave_total = level_words + LEVEL_U8_WAVE_WORD;
    uint8_t* __restrict__ raw = (uint8_t*)(level_words + LEVEL_U8_RAW_WORD);
    const uint8_t* __restrict__ x = (const uint8_t*)a.in;
    uint8_t* __restrict__ out = (uint8_t*)a.out;
    const int32_t window = a.window, lead = level_lead(window);
    const int32_t n_stage = LEVEL_U8_TILE + window - 1;         // <= LEVEL_U8_CAP; the whole tile's samples, also for a short last tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t i0 = tile * (int64_t)LEVEL_U8_TILE;
        const int32_t n_out = (int32_t)(a.out_len - i0 < LEVEL_U8_TILE ? a.out_len - i0 : LEVEL_U8_TILE);
        const int64_t g0 = a.in_start + i0 - lead;               // the tile's first sample (may lie outside the row)
        // 1. stage, four samples a thread in flight
        for (int32_t e0 = tid; e0 < n_stage; e0 += 4 * LEVEL_THREADS) {
            uint8_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (e0 + u * LEVEL_THREADS < n_stage) v[u] = row_at(x, a.n_in, g0 + e0 + u * LEVEL_THREADS);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int32_t e = e0 + u * LEVEL_THREADS;
                if (e < n_stage) raw[e] = v[u];
            }
        }
        __syncthreads();
        // 2. the prefix sums: a thread's chunk, the wave's scan of the chunks' totals, the waves' totals
        const int32_t e0 = tid * LEVEL_U8_CHUNK;
        uint32_t run[LEVEL_U8_CHUNK];
        uint32_t total = 0;
#pragma unroll
        for (int k = 0; k < LEVEL_U8_CHUNK; ++k) {
            total += e0 + k < n_stage ? (uint32_t)level_abs(row_deviation(raw[e0 + k])) : 0u;
            run[k] = total;
        }
        uint32_t incl = total;                                   // the inclusive scan of `total` over the wave's lanes
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
            const uint32_t up = (uint32_t)__shfl_up((int)incl, step, 64);
            incl += lane >= step ? up : 0u;
        }
        if (lane == 63) wave_total[wave] = incl;
        __syncthreads();
        uint32_t base = incl - total;
#pragma unroll
        for (int v = 0; v < LEVEL_THREADS / 64 - 1; ++v) base += v < wave ? wave_total[v] : 0u;
        if (tid == 0) prefix[0] = 0u;
#pragma unroll
        for (int k = 0; k < LEVEL_U8_CHUNK; ++k) prefix[e0 + k + 1] = base + run[k];
        __syncthreads();
        // 3. outputs, LEVEL_THREADS apart
#pragma unroll 4
        for (int r = 0; r < LEVEL_U8_PER; ++r) {
            const int32_t i = r * LEVEL_THREADS + tid;
            if (i < n_out) {
                const int32_t e = (int32_t)(prefix[i + window] - prefix[i]);
                out[i0 + i] = level_output<uint8_t>(row_deviation(raw[i + lead]), e, window, a.fw, a.peak);
            }
        }
        __syncthreads();                                    // the next tile stages over what this one read
    }
}

void launch(const LevelArgs& a, const LevelStage& s, hipStream_t st, uint8_t) {
    hipLaunchKernelGGL(level_u8_kernel, dim3(s.grid), dim3(LEVEL_THREADS), s.lds_bytes, st, a);
}
void launch(const LevelArgs& a, const LevelStage& s, hipStream_t st, float) {
    hipLaunchKernelGGL(level_f32_kernel, dim3(s.grid), dim3(LEVEL_THREADS), s.lds_bytes, st, a);
}

}  // namespace

extern "C" {

int sushi_hip_level(const void* in_dev, int dtype, int64_t n_in, int64_t in_start, int32_t window, double floor_, double peak,
                    void* out_dev, int64_t out_len, void* hip_stream) { return c_boundary([&]() -> int {
    LevelStage staged;
    const int rc = stage_level(in_dev, dtype, n_in, in_start, window, floor_, peak, out_dev, out_len, staged);
    if (rc != SUSHI_HIP_OK) return rc;

    LevelArgs a;
    a.in = in_dev; a.n_in = n_in; a.in_start = in_start; a.window = window; a.n_tiles = staged.n_tiles;
    a.peak = peak; a.out = out_dev; a.out_len = out_len;
    row_dispatch(dtype, [&](auto t) {
        a.fw = level_floor_term<decltype(t)>(floor_, window);
        launch(a, staged, (hipStream_t)hip_stream, t);
    });
    return launch_ok();
}); }

}  // extern "C"
