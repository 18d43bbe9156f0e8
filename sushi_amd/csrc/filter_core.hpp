// sushi_amd/csrc/filter_core.hpp -- the arithmetic of sushi_hip_filter (include/sushi_hip.h "FIR filter"): a row
// correlated with T float64 taps about the sample type's nominal centre, one output per sample.
// Plain C++: sushi_filter.hip runs it on the device, tests/host_filter_check.cpp on the CPU (g++).  Both are compiled with
// -ffp-contract=off: every product and every addition rounds once, the additions in ascending tap order, as NumPy's do.
// Behind it, host only: stage_filter -- the arguments of a call -> a refusal, or the tile, the tile count and the grid.
#ifndef SUSHI_FILTER_CORE_HPP
#define SUSHI_FILTER_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "row_core.hpp"            // row_at, row_deviation, row_call_ok

namespace sushi {

constexpr int32_t FILTER_MAX_TAPS = 2047;                    // T: odd, 1 .. 2047

// x - c, c = sushi_hip_centre, as a float64 (row_deviation: one float64 subtraction, or exact).
template <class T>
SUSHI_GEOM_HD inline double filter_deviation(T x) { return (double)row_deviation(x); }

// Samples in front of output i that h[0] meets: a = (T - 1) / 2.
SUSHI_GEOM_HD inline int32_t filter_lead(int32_t n_taps) { return (n_taps - 1) / 2; }

// One step of an output's sum: the product rounds, then the sum.
SUSHI_GEOM_HD inline double filter_step(double acc, double h, double d) {
    const double p = h * d;
    return acc + p;
}

// acc -> the output sample.  float32: (float)(acc + 0.5).  uint8: floor(acc + 128.5) held to 0 .. 255; both comparisons fail for a
// NaN, which so gives 0.
SUSHI_GEOM_HD inline float filter_finish(double acc, const float*) { return (float)(acc + 0.5); }
SUSHI_GEOM_HD inline uint8_t filter_finish(double acc, const uint8_t*) {
    const double v = floor(acc + 128.5);
    return v >= 255.0 ? (uint8_t)255 : (v >= 0.0 ? (uint8_t)v : (uint8_t)0);
}

// One output straight from the row (the CPU check; the kernel forms the same sum, in the same order, from its staged tile).
template <class T>
inline T filter_sample(const T* x, int64_t n_in, int64_t in_start, const double* taps, int32_t n_taps, int64_t i) {
    const int64_t g0 = in_start + i - filter_lead(n_taps);
    double acc = 0.0;
    for (int32_t k = 0; k < n_taps; ++k) acc = filter_step(acc, taps[k], filter_deviation(row_at(x, n_in, g0 + k)));
    return filter_finish(acc, (const T*)0);
}

// ---- the tile of a workgroup ----
// FILTER_THREADS threads own `per` consecutive outputs each: 8 up to 1025 taps, 4 above (the halo of T - 1 samples must fit beside
// the tile).  The workgroup stages the tile's tile + T - 1 deviations as float64, and the taps.  Element e of the staged samples
// lies in slot e + e / per: a thread's window starts per + 1 doubles behind its neighbour's, an odd stride, so that the lanes of a
// read that walk their windows in step meet different LDS banks.
constexpr int FILTER_THREADS = 256;
constexpr int32_t FILTER_WIDE = 8, FILTER_NARROW = 4;         // outputs a thread
constexpr int32_t FILTER_WIDE_MAX_TAPS = 1025;
constexpr int32_t FILTER_CUS = 256, FILTER_CU_LDS = 160 * 1024;
constexpr int32_t FILTER_MAX_RESIDENT = 5;                     // workgroups a CU holds by registers (a wave of each on every SIMD)

SUSHI_GEOM_HD constexpr int32_t filter_per_thread(int32_t n_taps) { return n_taps <= FILTER_WIDE_MAX_TAPS ? FILTER_WIDE : FILTER_NARROW; }
SUSHI_GEOM_HD constexpr int32_t filter_tile(int32_t n_taps) { return FILTER_THREADS * filter_per_thread(n_taps); }
SUSHI_GEOM_HD constexpr int32_t filter_slot(int32_t e, int32_t per) { return e + e / per; }
// slots a tile's staged samples take at T taps
SUSHI_GEOM_HD constexpr int32_t filter_slots(int32_t n_taps) {
    return filter_slot(filter_tile(n_taps) + n_taps - 2, filter_per_thread(n_taps)) + 1;
}
// The LDS of a workgroup, sized by the call: the taps first (T + 1 doubles: what follows stays 16-byte aligned), then the slots.
SUSHI_GEOM_HD constexpr int32_t filter_lds_bytes(int32_t n_taps) { return (n_taps + 1 + filter_slots(n_taps)) * 8; }
// (within either kind of tile the need grows with T)
static_assert(filter_lds_bytes(FILTER_WIDE_MAX_TAPS) <= 48 * 1024 && filter_lds_bytes(FILTER_MAX_TAPS) <= 48 * 1024,
              "a tile's samples and the taps fit 48 KB of LDS: at least three workgroups to a CU");
// A fixed grid striding over the tiles: as many workgroups as the CUs hold at once, by LDS and by registers.
SUSHI_GEOM_HD constexpr int32_t filter_resident(int32_t n_taps) {
    return FILTER_CU_LDS / filter_lds_bytes(n_taps) < FILTER_MAX_RESIDENT ? FILTER_CU_LDS / filter_lds_bytes(n_taps) : FILTER_MAX_RESIDENT;
}

// ---- the host side of a call ----
struct FilterStage {
    int32_t tile;             // outputs per tile
    int64_t n_tiles;
    unsigned grid;
    unsigned lds_bytes;       // dynamic LDS of the launch
};

// EINVAL: an unknown dtype, n_in < 1 (or >= 2^62), in_start outside [0, n_in - 1], out_len outside 1 .. 2^40 - 1, T even or
// outside 1 .. 2047, a null pointer (`out` is then unspecified).
inline int stage_filter(const void* x, int dtype, int64_t n_in, int64_t in_start, const void* taps, int32_t n_taps,
                        const void* y, int64_t out_len, FilterStage& out) {
    if (!x || !taps || !y) return SUSHI_HIP_EINVAL;
    if (row_call_ok(dtype, n_in, in_start, out_len) != SUSHI_HIP_OK) return SUSHI_HIP_EINVAL;
    if (n_taps < 1 || n_taps > FILTER_MAX_TAPS || !(n_taps & 1)) return SUSHI_HIP_EINVAL;
    out.tile = filter_tile(n_taps);
    out.n_tiles = (out_len + out.tile - 1) / out.tile;
    const int64_t most = (int64_t)FILTER_CUS * filter_resident(n_taps);
    out.grid = (unsigned)(out.n_tiles < most ? out.n_tiles : most);
    out.lds_bytes = (unsigned)filter_lds_bytes(n_taps);
    return SUSHI_HIP_OK;
}

}  // namespace sushi
#endif
