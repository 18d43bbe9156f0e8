// sushi_amd/csrc/row_core.hpp -- what the calls that read a row of samples and write another have in common:
// retime, envelope and filter, the load pipeline's resample, and the sample type of a stream.  The sample type of a call; a row's
// sample with both clamps; its deviation from the type's nominal centre; the refusals every row call opens with; the cursor of a
// rational step.  Plain C++: the cores that include it are compiled by hipcc for the library and by g++ for their CPU checks.
#ifndef SUSHI_ROW_CORE_HPP
#define SUSHI_ROW_CORE_HPP

#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_geometry.hpp"      // SUSHI_GEOM_HD

namespace sushi {

constexpr int64_t ROW_MAX_LEN = (int64_t)1 << 40;          // outputs of a call (i * num, num <= 2^20, stays below 2^60)
constexpr int64_t ROW_MAX_IN = (int64_t)1 << 62;           // n_in (in_start + an output's reach stays inside int64)

// ---- the sample type of a call (host) ----
inline bool row_dtype_ok(int dtype) { return dtype == SUSHI_HIP_U8 || dtype == SUSHI_HIP_F32; }
inline int row_sample_size(int dtype) { return dtype == SUSHI_HIP_U8 ? 1 : 4; }
// a pointer to samples lies on a multiple of the sample's size (what SUSHI_HIP_EALIGN refuses otherwise)
inline bool row_aligned(const void* p, int dtype) { return !((uintptr_t)p & (uintptr_t)(row_sample_size(dtype) - 1)); }
// f(a value of the sample type): f is a generic lambda, decltype of its argument names the kernel's T
template <class F>
inline void row_dispatch(int dtype, F f) {
    if (dtype == SUSHI_HIP_U8) f(uint8_t());
    else f(float());
}

// EINVAL: an unknown dtype, n_in < 1 (or >= 2^62), in_start outside [0, n_in - 1], out_len outside 1 .. 2^40 - 1.
inline int row_call_ok(int dtype, int64_t n_in, int64_t in_start, int64_t out_len) {
    if (!row_dtype_ok(dtype)) return SUSHI_HIP_EINVAL;
    if (n_in < 1 || n_in >= ROW_MAX_IN) return SUSHI_HIP_EINVAL;
    if (in_start < 0 || in_start > n_in - 1) return SUSHI_HIP_EINVAL;
    if (out_len < 1 || out_len >= ROW_MAX_LEN) return SUSHI_HIP_EINVAL;
    return SUSHI_HIP_OK;
}

// ---- a sample ----
// The row's sample at index g with both clamps.
template <class T>
SUSHI_GEOM_HD inline T row_at(const T* x, int64_t n_in, int64_t g) { return x[g < 0 ? 0 : (g < n_in ? g : n_in - 1)]; }

// x - c, c = sushi_hip_centre: 0.5 (one float64 subtraction) or 128 (exact, an integer).
SUSHI_GEOM_HD inline double row_deviation(float x) { return (double)x - 0.5; }
SUSHI_GEOM_HD inline int32_t row_deviation(uint8_t x) { return (int32_t)x - 128; }

// ---- a rational step ----
// Where output i of a run that starts at sample j0 and takes num / den input samples per output stands: at sample j and the
// fraction r / den behind it.
struct RowCursor {
    int64_t j;
    int32_t r;            // 0 <= r < den
};

// The one 64-bit division of a run of outputs: t = i * num, j = j0 + t / den, r = t % den  (i < 2^40, num <= 2^20: no overflow).
SUSHI_GEOM_HD inline RowCursor row_seek(int64_t j0, int64_t i, int32_t num, int32_t den) {
    const uint64_t t = (uint64_t)i * (uint64_t)num;
    const uint64_t q = t / (uint32_t)den;
    RowCursor c;
    c.j = j0 + (int64_t)q;
    c.r = (int32_t)(t - q * (uint32_t)den);
    return c;
}

// ... and on by a fixed number of outputs without another: (qstep, rstep) = divmod(outputs * num, den); the carry goes into j.
SUSHI_GEOM_HD inline void row_advance(RowCursor& c, int32_t qstep, int32_t rstep, int32_t den) {
    c.r += rstep;
    c.j += qstep;
    if (c.r >= den) { c.r -= den; c.j += 1; }
}

}  // namespace sushi
#endif
