// sushi_amd/csrc/retime_core.hpp -- the arithmetic of sushi_hip_retime (include/sushi_hip.h "retiming"), one sample
// at a time.  Plain C++: sushi_retime.hip runs it on the device, tests/host_retime_check.cpp on the CPU (g++).  Both are compiled
// with -ffp-contract=off: the product and the sum of the interpolation round separately, as NumPy's do.
#ifndef SUSHI_RETIME_CORE_HPP
#define SUSHI_RETIME_CORE_HPP

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RETIME_HD __host__ __device__
#else
#define RETIME_HD
#endif

namespace sushi {

// Where output i of a segment reads its input: position in_start + i * num / den = sample j and the fraction r / den behind it.
struct RetimeCursor {
    int64_t j;
    int32_t r;            // 0 <= r < den
};

// The one 64-bit division of a run of outputs: t = i * num, j = in_start + t / den, r = t % den  (i < 2^40, num <= 2^20: no overflow).
RETIME_HD inline RetimeCursor retime_seek(int64_t in_start, int64_t i, int32_t num, int32_t den) {
    const uint64_t t = (uint64_t)i * (uint64_t)num;
    const uint64_t q = t / (uint32_t)den;
    RetimeCursor c;
    c.j = in_start + (int64_t)q;
    c.r = (int32_t)(t - q * (uint32_t)den);
    return c;
}

// ... and from output i to output i + 1 without another: r += num % den, the carry and num / den go into j.
RETIME_HD inline void retime_advance(RetimeCursor& c, int32_t qstep, int32_t rstep, int32_t den) {
    c.r += rstep;
    c.j += qstep;
    if (c.r >= den) { c.r -= den; c.j += 1; }
}

RETIME_HD inline float retime_round(double y, const float*) { return (float)y; }
RETIME_HD inline uint8_t retime_round(double y, const uint8_t*) { return (uint8_t)(y + 0.5); }       // half up (y >= 0)

// One output sample (T: float or uint8_t): y = x[j] + w * (x[j1] - x[j]) in float64, w = r / den, j1 = min(j + 1, n_in - 1);
// float32: (float)y; uint8: (uint8_t)(y + 0.5).
template <class T>
RETIME_HD inline T retime_sample(const T* x, int64_t n_in, int64_t j, int32_t r, int32_t den) {
    const int64_t j1 = j + 1 < n_in - 1 ? j + 1 : n_in - 1;
    const double a = (double)x[j];
    const double b = (double)x[j1];
    const double w = (double)r / (double)den;
    const double d = b - a;
    const double p = w * d;
    const double y = a + p;
    return retime_round(y, (const T*)0);
}

}  // namespace sushi
#endif
