// sushi_amd/csrc/sushi_resample.hip -- sushi_hip_load_resample_fir: a low-pass in front of the load pipeline's decimator (gfx950).
//
// A zero-phase polyphase FIR filter at the file's frame rate, in the arithmetic include/sushi_hip.h states and resample_core.hpp
// implements (float64, a tap's product and the running sum rounded separately: this unit is compiled with -ffp-contract=off), so
// that the row is bit-identical to the NumPy restatement (sushi_amd/resample.py resample_host).
//
// fir_body_kernel: a workgroup owns runs of `run` consecutive body samples (a fixed grid strides over the runs).  Per run it
// stages the input span the run reads -- ceil((run - 1) * num / den) + 2W samples, clamped at both ends of the input, widened to
// float64 once -- into LDS with coalesced loads, then every thread forms outputs i0 + tid, i0 + tid + 256, ...: one 64-bit
// division per thread and run (resample_seek), the rest by resample_advance.  Stores are coalesced.
//   * The span's LDS layout.  A wave's lanes read samples num / den apart.  At an integer step s (den == 1) that is a stride of
//     s float64 = 2s banks: a 4-way conflict at s = 4, 8-way at s = 8 (ds_read_b64: 64 banks, groups of 32 lanes).  So the span
//     is stored by phase: sample m at [m % s][m / s].  Tap c of lane l then reads [c % s][l + c / s]: one phase row for the whole
//     wave, consecutive float64 across the lanes, no conflict.  At a rational step the span lies as it is (LINEAR).
//   * The table row.  den == 1: one row for everyone, read through the scalar cache (UNIFORM: the address does not depend on
//     the lane).  Otherwise the rows go to LDS once per workgroup, at an odd stride in float64 so that 32 rows start on 32
//     different bank pairs (ROWS_LDS) -- or, when table and span do not fit 64 KB together, stay in global memory and are read
//     per lane out of L2 (ROWS_GLOBAL: 441/80 is 125 KB of table).
//   * Steps whose span does not fit LDS even for a run of 64 outputs (num / den in the hundreds) read the input directly
//     (DIRECT), clamped per tap.
// fir_edges_kernel then writes the zeros behind the body and both pads from the body's first and last sample.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "resample_core.hpp"

namespace {

using sushi::launch_ok;

constexpr int FIR_THREADS = 256;
constexpr int FIR_LDS_BYTES = 64 << 10;          // what a launch may ask for without opting in to more
constexpr int FIR_MAX_RUN = 1024;                // outputs per run: 4 per thread
constexpr int FIR_MIN_RUN = 64;
constexpr bool FIR_PHASE_LAYOUT = true;          // integer steps: the span by phase (false: as it lies; tools/experiments)

enum XMode { X_PHASES = 0, X_LINEAR = 1, X_DIRECT = 2 };
enum HMode { H_UNIFORM = 0, H_ROWS_LDS = 1, H_ROWS_GLOBAL = 2 };

struct FirArgs {
    const float* raw;
    int64_t n_raw;
    const double* table;      // [den][2W]
    float* data;
    int64_t n_body, pad, total, n_runs;
    int32_t num, den, W, run;
    int32_t xstride;          // X_PHASES: float64 per phase row
    int32_t hstride;          // H_ROWS_LDS: float64 per table row in LDS (odd)
    int32_t h_doubles;        // float64 of LDS in front of the span (the table's rows)
    int32_t reserved;
};

template <int XMODE, int HMODE>
__global__ __launch_bounds__(FIR_THREADS)
void fir_body_kernel(FirArgs a) {
    extern __shared__ double fir_lds[];
    double* __restrict__ hl = fir_lds;
    double* __restrict__ xl = fir_lds + a.h_doubles;
    const float* __restrict__ raw = a.raw;
    // the table is read only: through the constant address space a lane-independent address becomes a scalar load
    typedef const double __attribute__((address_space(4))) ConstDouble;
    ConstDouble* __restrict__ table = (ConstDouble*)(uintptr_t)a.table;
    float* __restrict__ data = a.data;
    const int32_t taps = 2 * a.W;
    const int tid = threadIdx.x;
    if (HMODE == H_ROWS_LDS) {
        for (int r = tid >> 6; r < a.den; r += FIR_THREADS >> 6)
            for (int c = tid & 63; c < taps; c += 64) hl[r * a.hstride + c] = table[(int64_t)r * taps + c];
    }
    // from a thread's output to its next one, FIR_THREADS further on
    const int64_t hop = (int64_t)FIR_THREADS * a.num;
    const int32_t qhop = (int32_t)(hop / a.den), rhop = (int32_t)(hop % a.den);
    for (int64_t run = blockIdx.x; run < a.n_runs; run += gridDim.x) {
        const int64_t i0 = run * a.run;
        const int64_t i1 = i0 + a.run < a.n_body ? i0 + a.run : a.n_body;
        const sushi::ResampleCursor c0 = sushi::resample_seek(i0, a.num, a.den);
        if (XMODE != X_DIRECT) {
            const int64_t base = c0.j - a.W + 1;                                   // the span's first sample (before clamping)
            const int32_t len = (int32_t)(sushi::resample_seek(i1 - 1, a.num, a.den).j - c0.j) + taps;
            __syncthreads();                                                       // the run before has been read
            for (int32_t m = tid; m < len; m += FIR_THREADS) {
                int64_t k = base + m;
                k = k < 0 ? 0 : (k > a.n_raw - 1 ? a.n_raw - 1 : k);
                const int32_t at = XMODE == X_PHASES ? (m % a.num) * a.xstride + m / a.num : m;
                xl[at] = (double)raw[k];
            }
        }
        if (XMODE != X_DIRECT || HMODE == H_ROWS_LDS) __syncthreads();
        if (i0 + tid >= i1) continue;
        sushi::ResampleCursor cur = sushi::resample_seek(i0 + tid, a.num, a.den);
        for (int64_t i = i0 + tid; i < i1; i += FIR_THREADS) {
            const int32_t off = (int32_t)(cur.j - c0.j);                           // the span's sample under tap 0
            ConstDouble* __restrict__ grow = HMODE == H_ROWS_GLOBAL ? table + (int64_t)cur.r * taps : table;
            const double* __restrict__ lrow = hl + cur.r * a.hstride;
            auto h = [&](int32_t c) { return HMODE == H_ROWS_LDS ? lrow[c] : grow[c]; };
            float y;
            if (XMODE == X_PHASES) {
                // off = (i - i0) * num: tap c lies in phase row c % num at (i - i0) + c / num
                const double* __restrict__ p = xl + (int32_t)(i - i0);
                int32_t phase = 0;
                y = sushi::resample_output(taps, [&](int32_t) {
                    const double v = p[phase * a.xstride];
                    if (++phase == a.num) { phase = 0; ++p; }
                    return v;
                }, h);
            } else if (XMODE == X_LINEAR) {
                const double* __restrict__ p = xl + off;
                y = sushi::resample_output(taps, [&](int32_t c) { return p[c]; }, h);
            } else {
                y = sushi::resample_output(taps, [&](int32_t c) {
                    return (double)raw[sushi::resample_tap_index(cur.j, a.W, c, a.n_raw)]; }, h);
            }
            data[a.pad + i] = y;
            sushi::resample_advance(cur, qhop, rhop, a.den);
        }
    }
}

// Everything of [0, total) outside the body: zeros behind it, and the pads (both read the body, which the kernel before wrote).
__global__ __launch_bounds__(256)
void fir_edges_kernel(float* __restrict__ data, int64_t n_body, int64_t pad, int64_t total) {
    const int64_t body_end = pad + n_body, inner_end = total - pad;
    const float left = data[pad];
    const float right = body_end == inner_end ? data[body_end - 1] : 0.f;          // data[total - pad - 1]
    const int64_t n_edge = total - n_body;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_edge; e += (int64_t)gridDim.x * 256) {
        const int64_t pos = e < pad ? e : e + n_body;
        data[pos] = pos < pad ? left : (pos < inner_end ? 0.f : right);
    }
}

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// How a step is served: the run, the LDS layout and its size.  False: the span does not fit LDS (DIRECT).
bool fir_plan(FirArgs& a, int& xmode, int& hmode, size_t& lds_bytes) {
    const int64_t taps = 2 * (int64_t)a.W;
    a.hstride = 0; a.h_doubles = 0; a.xstride = 0;
    hmode = a.den == 1 ? H_UNIFORM : H_ROWS_GLOBAL;
    const bool phases = a.den == 1 && FIR_PHASE_LAYOUT;
    auto span_doubles = [&](int64_t run, int32_t* xstride) -> int64_t {
        const int64_t span = ceil_div((run - 1) * a.num, a.den) + taps;
        if (!phases) return span;
        int64_t rows = ceil_div(span, a.num);
        const int64_t want = a.num <= 16 ? 16 / a.num : 1;       // rows start 16 / s bank pairs apart: the staging stores spread too
        while (rows % 16 != want % 16) ++rows;
        *xstride = (int32_t)rows;
        return rows * a.num;
    };
    const int64_t budget = FIR_LDS_BYTES / 8;
    if (a.den > 1) {
        const int64_t hstride = taps | 1;
        // the rows go to LDS if a run of 256 outputs still fits beside them
        if (a.den * hstride + span_doubles(256, nullptr) <= budget) {
            hmode = H_ROWS_LDS;
            a.hstride = (int32_t)hstride;
            a.h_doubles = (int32_t)(a.den * hstride);
        }
    }
    for (int run = FIR_MAX_RUN; run >= FIR_MIN_RUN; run >>= 1) {
        int32_t xstride = 0;
        const int64_t need = a.h_doubles + span_doubles(run, &xstride);
        if (need <= budget) {
            a.run = run;
            a.xstride = xstride;
            xmode = phases ? X_PHASES : X_LINEAR;
            lds_bytes = (size_t)need * 8;
            return true;
        }
    }
    a.run = FIR_THREADS;
    xmode = X_DIRECT;
    lds_bytes = 0;
    return false;
}

template <int XMODE, int HMODE>
void fir_launch(const FirArgs& a, unsigned grid, size_t lds_bytes, hipStream_t st) {
    hipLaunchKernelGGL((fir_body_kernel<XMODE, HMODE>), dim3(grid), dim3(FIR_THREADS), lds_bytes, st, a);
}

}  // namespace

extern "C" {

int sushi_hip_load_resample_fir(const float* raw_dev, int64_t n_raw, int32_t num, int32_t den, const double* table_dev,
                                int32_t half_width, int64_t n_body, int64_t pad, int64_t total, float* data_dev, void* hip_stream) {
    if (!raw_dev || !table_dev || !data_dev) return SUSHI_HIP_EINVAL;
    if (n_raw < 1 || n_body < 1 || n_body >= sushi::RESAMPLE_MAX_BODY) return SUSHI_HIP_EINVAL;
    if (num < 1 || num > sushi::RESAMPLE_MAX_TERM || den < 1 || den > sushi::RESAMPLE_MAX_TERM) return SUSHI_HIP_EINVAL;
    if (half_width < 1 || (int64_t)den * 2 * (int64_t)half_width > sushi::RESAMPLE_MAX_TABLE) return SUSHI_HIP_EINVAL;
    if ((n_body - 1) * (int64_t)num / den > n_raw - 1) return SUSHI_HIP_EINVAL;                    // the last read's centre
    if (pad < 0 || total < 0 || pad > total || n_body > total - pad || pad + n_body > total - pad) return SUSHI_HIP_EINVAL;
    if (((uintptr_t)table_dev & 7) || ((uintptr_t)raw_dev & 3) || ((uintptr_t)data_dev & 3)) return SUSHI_HIP_EALIGN;

    FirArgs a;
    a.raw = raw_dev; a.n_raw = n_raw; a.table = table_dev; a.data = data_dev;
    a.n_body = n_body; a.pad = pad; a.total = total;
    a.num = num; a.den = den; a.W = half_width; a.reserved = 0;
    int xmode, hmode;
    size_t lds_bytes;
    fir_plan(a, xmode, hmode, lds_bytes);
    if (xmode == X_DIRECT && hmode == H_ROWS_LDS) { hmode = H_ROWS_GLOBAL; a.hstride = 0; a.h_doubles = 0; }
    a.n_runs = (n_body + a.run - 1) / a.run;
    // a fixed grid striding over the runs: 256 CUs, up to eight workgroups each
    const unsigned grid = (unsigned)(a.n_runs < 2048 ? a.n_runs : 2048);
    hipStream_t st = (hipStream_t)hip_stream;
    if (xmode == X_PHASES) fir_launch<X_PHASES, H_UNIFORM>(a, grid, lds_bytes, st);
    else if (xmode == X_LINEAR && hmode == H_UNIFORM) fir_launch<X_LINEAR, H_UNIFORM>(a, grid, lds_bytes, st);
    else if (xmode == X_LINEAR && hmode == H_ROWS_LDS) fir_launch<X_LINEAR, H_ROWS_LDS>(a, grid, lds_bytes, st);
    else if (xmode == X_LINEAR) fir_launch<X_LINEAR, H_ROWS_GLOBAL>(a, grid, lds_bytes, st);
    else if (hmode == H_UNIFORM) fir_launch<X_DIRECT, H_UNIFORM>(a, grid, 0, st);
    else fir_launch<X_DIRECT, H_ROWS_GLOBAL>(a, grid, 0, st);
    if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    const int64_t n_edge = total - n_body;
    if (n_edge > 0) {
        const int64_t want = (n_edge + 255) / 256;
        hipLaunchKernelGGL(fir_edges_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, st, data_dev, n_body, pad, total);
    }
    return launch_ok();
}

}  // extern "C"
