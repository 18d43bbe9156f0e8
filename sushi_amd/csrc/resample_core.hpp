// sushi_amd/csrc/resample_core.hpp -- the arithmetic of sushi_hip_load_resample_fir (include/sushi_hip.h "filtered decimation";
// DESIGN.md 3.14), one output at a time.  Plain C++: sushi_resample.hip runs it on the device, tests/host_resample_check.cpp on
// the CPU (g++).  Both are compiled with -ffp-contract=off: a tap's product and the running sum round separately, as NumPy's do.
#ifndef SUSHI_RESAMPLE_CORE_HPP
#define SUSHI_RESAMPLE_CORE_HPP

#include <stdint.h>

#include "row_core.hpp"            // the cursor of a rational step, ROW_MAX_LEN

namespace sushi {

constexpr int32_t RESAMPLE_MAX_TERM = 1 << 20;              // num, den
constexpr int64_t RESAMPLE_MAX_TABLE = 65536;               // den * 2W table entries
constexpr int64_t RESAMPLE_MAX_BODY = ROW_MAX_LEN;          // n_body (i * num stays below 2^60)

// Where body sample i reads its input: the filter is centred on i * num / den = sample j and the fraction r / den behind it;
// r picks the table's row.  One division per run of outputs, then advances by a fixed number of outputs (row_core.hpp).
typedef RowCursor ResampleCursor;
SUSHI_GEOM_HD inline ResampleCursor resample_seek(int64_t i, int32_t num, int32_t den) { return row_seek(0, i, num, den); }
SUSHI_GEOM_HD inline void resample_advance(ResampleCursor& c, int32_t qstep, int32_t rstep, int32_t den) { row_advance(c, qstep, rstep, den); }

// The sample tap c of an output centred on j reads: x[clamp(j - W + 1 + c, 0, n_raw - 1)].
SUSHI_GEOM_HD inline int64_t resample_tap_index(int64_t j, int32_t half_width, int32_t c, int64_t n_raw) {
    const int64_t k = j - half_width + 1 + c;
    return k < 0 ? 0 : (k > n_raw - 1 ? n_raw - 1 : k);
}

// One output: acc = 0.0; for c = 0 .. taps - 1 in that order acc = acc + h(c) * x(c) in float64, product and sum rounded
// separately; y = (float)acc.  x(c): tap c's input sample as a double (the float32 sample, widened); h(c): H[r][c].  Both are
// called once per tap, in ascending c.
template <class X, class H>
SUSHI_GEOM_HD inline float resample_output(int32_t taps, X x, H h) {
    double acc = 0.0;
#if defined(__clang__)
#pragma unroll 8
#endif
    for (int32_t c = 0; c < taps; ++c) {
        const double p = h(c) * x(c);
        acc = acc + p;
    }
    return (float)acc;
}

}  // namespace sushi
#endif
