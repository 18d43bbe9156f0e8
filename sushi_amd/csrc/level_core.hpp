// sushi_amd/csrc/level_core.hpp -- the arithmetic of sushi_hip_level (include/sushi_hip.h "levelling"): every sample's
// deviation from the sample type's nominal centre divided by the local level, the mean absolute deviation over W samples around it.
// Plain C++: sushi_level.hip runs it on the device, tests/host_level_check.cpp on the CPU (g++).  Both are compiled with
// -ffp-contract=off: the float32 window sum is sequential in ascending t, every addition rounded once, as NumPy's; the uint8 window
// sum is an exact integer, whichever way it is formed.
// Behind it, host only: stage_level -- the arguments of a call -> a refusal, or the tile, the tile count, the grid and the LDS.
#ifndef SUSHI_LEVEL_CORE_HPP
#define SUSHI_LEVEL_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "row_core.hpp"            // row_at, row_deviation, row_call_ok, row_aligned

namespace sushi {

constexpr int32_t LEVEL_MAX_WINDOW = 1023;                    // W: odd, 1 .. 1023

// What a window's sum of |d| is kept in: float64 for float32 samples, an integer for uint8 (at most 1023 * 128 = 130944).
template <class T> struct LevelSum;
template <> struct LevelSum<float> { typedef double type; };
template <> struct LevelSum<uint8_t> { typedef int32_t type; };

// |d| of a deviation (row_deviation's: a float64, or an exact integer)
SUSHI_GEOM_HD inline double level_abs(double d) { return fabs(d); }
SUSHI_GEOM_HD inline int32_t level_abs(int32_t d) { return d < 0 ? -d : d; }

// H, the sample type's half range
SUSHI_GEOM_HD inline double level_half_range(const float*) { return 0.5; }
SUSHI_GEOM_HD inline double level_half_range(const uint8_t*) { return 128.0; }

// Samples in front of output i that the window starts: h = (W - 1) / 2.
SUSHI_GEOM_HD inline int32_t level_lead(int32_t window) { return (window - 1) / 2; }

// fw = (floor * H) * (double)W: two float64 multiplications, in that order.
template <class T>
SUSHI_GEOM_HD inline double level_floor_term(double floor_, int32_t window) {
    const double fh = floor_ * level_half_range((const T*)0);
    return fh * (double)window;
}

// q of an output from its deviation d, its window sum e and fw: den = (e + fw) * peak; q = (d * W) / den -- one sum, two products
// and one division, each rounded once; a NaN q (0 / 0, inf / inf, a NaN sample) becomes 0; then q is held to [-1, 1].
SUSHI_GEOM_HD inline double level_quotient(double d, int32_t window, double e, double fw, double peak) {
    const double sum = e + fw;
    const double den = sum * peak;
    const double num = d * (double)window;
    double q = num / den;
    q = q == q ? q : 0.0;
    return q > 1.0 ? 1.0 : (q < -1.0 ? -1.0 : q);
}

// q -> the output sample.  float32: (float)(0.5 + 0.5 * q).  uint8: floor(q * 128.0 + 128.5), at least 0 as q >= -1, held to 255
// (q = 1 gives 256).
SUSHI_GEOM_HD inline float level_finish(double q, const float*) {
    const double half = 0.5 * q;
    return (float)(0.5 + half);
}
SUSHI_GEOM_HD inline uint8_t level_finish(double q, const uint8_t*) {
    const int32_t v = (int32_t)floor(q * 128.0 + 128.5);
    return (uint8_t)(v < 255 ? v : 255);
}

// An output from its deviation and window sum, whatever they were kept in.
template <class T, class D, class S>
SUSHI_GEOM_HD inline T level_output(D d, S e, int32_t window, double fw, double peak) {
    return level_finish(level_quotient((double)d, window, (double)e, fw, peak), (const T*)0);
}

// What output i has of the row, straight from it with both clamps: its deviation d and its window sum e, t = 0 .. W - 1 in that
// order (the CPU check; the kernels form the same sum -- float32: in the same order -- from their staged tile).
template <class T>
struct LevelWindow {
    decltype(row_deviation(T())) d;
    typename LevelSum<T>::type e;
};
template <class T>
inline LevelWindow<T> level_window(const T* x, int64_t n_in, int64_t in_start, int32_t window, int64_t i) {
    const int64_t g = in_start + i, g0 = g - level_lead(window);
    LevelWindow<T> w;
    w.d = row_deviation(row_at(x, n_in, g));
    w.e = 0;
    for (int32_t t = 0; t < window; ++t) w.e = w.e + level_abs(row_deviation(row_at(x, n_in, g0 + t)));
    return w;
}

// One output straight from the row.
template <class T>
inline T level_sample(const T* x, int64_t n_in, int64_t in_start, int32_t window, double floor_, double peak, int64_t i) {
    const LevelWindow<T> w = level_window(x, n_in, in_start, window, i);
    return level_output<T>(w.d, w.e, window, level_floor_term<T>(floor_, window), peak);
}

// ---- the tile of a workgroup ----
// LEVEL_THREADS threads own a tile of consecutive outputs and stage its tile + W - 1 samples in LDS.
constexpr int LEVEL_THREADS = 256;
constexpr int32_t LEVEL_CUS = 256, LEVEL_CU_LDS = 160 * 1024;
constexpr int32_t LEVEL_MAX_RESIDENT = 4;                      // workgroups of 256 threads a CU is given at the most

// float32 -- the tile of filter_kernel: LEVEL_F32_PER consecutive outputs a thread, the deviations staged as float64, element e in
// slot e + e / PER: a thread's window starts PER + 1 doubles behind its neighbour's, an odd stride, so that the lanes of a read
// that walk their windows in step meet different LDS banks.  The LDS of a workgroup is sized by the call.
constexpr int32_t LEVEL_F32_PER = 8;
constexpr int32_t LEVEL_F32_TILE = LEVEL_THREADS * LEVEL_F32_PER;
SUSHI_GEOM_HD constexpr int32_t level_f32_slot(int32_t e) { return e + e / LEVEL_F32_PER; }
SUSHI_GEOM_HD constexpr int32_t level_f32_lds_bytes(int32_t window) { return (level_f32_slot(LEVEL_F32_TILE + window - 2) + 1) * 8; }
static_assert(level_f32_lds_bytes(LEVEL_MAX_WINDOW) <= 32 * 1024, "a float32 tile's samples fit 32 KB of LDS: four workgroups to a CU and room to spare");

// uint8 -- a thread scans LEVEL_U8_CHUNK consecutive staged samples (an odd number: its words of the prefix sum lie an odd stride
// from its neighbour's) and finishes LEVEL_U8_PER outputs LEVEL_THREADS apart.  The LDS, the same for every window, in 32-bit
// words: P[0 .. CAP], the prefix sums (P[k]: the sum of |d| of the tile's first k staged samples); the four waves' totals; from
// LEVEL_U8_RAW_WORD on, the CAP staged bytes.
constexpr int32_t LEVEL_U8_PER = 16;
constexpr int32_t LEVEL_U8_TILE = LEVEL_THREADS * LEVEL_U8_PER;
constexpr int32_t LEVEL_U8_CHUNK = 21;
constexpr int32_t LEVEL_U8_CAP = LEVEL_THREADS * LEVEL_U8_CHUNK;
constexpr int32_t LEVEL_U8_WAVE_WORD = LEVEL_U8_CAP + 1;
constexpr int32_t LEVEL_U8_RAW_WORD = LEVEL_U8_CAP + 8;
constexpr int32_t LEVEL_U8_LDS_BYTES = LEVEL_U8_RAW_WORD * 4 + LEVEL_U8_CAP;
static_assert(LEVEL_U8_TILE + LEVEL_MAX_WINDOW - 1 <= LEVEL_U8_CAP, "the threads' chunks cover a tile's staged samples at the widest window");
static_assert(LEVEL_U8_LDS_BYTES <= 32 * 1024, "a uint8 tile's bytes and prefix sums fit 32 KB of LDS");

// ---- the host side of a call ----
struct LevelStage {
    int32_t tile;             // outputs per tile
    int64_t n_tiles;
    unsigned grid;            // a fixed grid striding over the tiles: as many workgroups as the CUs are given at once
    unsigned lds_bytes;       // dynamic LDS of the launch
};

// finite and > 0 (a NaN fails both comparisons)
inline bool level_positive(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

inline int32_t level_tile(int dtype) { return dtype == SUSHI_HIP_U8 ? LEVEL_U8_TILE : LEVEL_F32_TILE; }
inline int32_t level_lds_bytes(int dtype, int32_t window) { return dtype == SUSHI_HIP_U8 ? LEVEL_U8_LDS_BYTES : level_f32_lds_bytes(window); }
inline int32_t level_resident(int dtype, int32_t window) {
    const int32_t by_lds = LEVEL_CU_LDS / level_lds_bytes(dtype, window);
    return by_lds < LEVEL_MAX_RESIDENT ? by_lds : LEVEL_MAX_RESIDENT;
}

// EINVAL: a null pointer, an unknown dtype, n_in < 1 (or >= 2^62), in_start outside [0, n_in - 1], out_len outside 1 .. 2^40 - 1,
// W even or outside 1 .. 1023, floor or peak not finite or not > 0; EALIGN: x or y not on a multiple of the sample's size (`out` is
// then unspecified).
inline int stage_level(const void* x, int dtype, int64_t n_in, int64_t in_start, int32_t window, double floor_, double peak,
                       const void* y, int64_t out_len, LevelStage& out) {
    if (!x || !y) return SUSHI_HIP_EINVAL;
    if (row_call_ok(dtype, n_in, in_start, out_len) != SUSHI_HIP_OK) return SUSHI_HIP_EINVAL;
    if (window < 1 || window > LEVEL_MAX_WINDOW || !(window & 1)) return SUSHI_HIP_EINVAL;
    if (!level_positive(floor_) || !level_positive(peak)) return SUSHI_HIP_EINVAL;
    if (!row_aligned(x, dtype) || !row_aligned(y, dtype)) return SUSHI_HIP_EALIGN;
    out.tile = level_tile(dtype);
    out.n_tiles = (out_len + out.tile - 1) / out.tile;
    const int64_t most = (int64_t)LEVEL_CUS * level_resident(dtype, window);
    out.grid = (unsigned)(out.n_tiles < most ? out.n_tiles : most);
    out.lds_bytes = (unsigned)level_lds_bytes(dtype, window);
    return SUSHI_HIP_OK;
}

}  // namespace sushi
#endif
