// sushi_amd/csrc/track_margin_device.hpp -- the device side the two margins passes share (sushi_track.hip's and
// sushi_track_order.hip's): the partial records of three first minima a step's workgroups leave, and how one workgroup turns
// them into a row's outputs.  Device code only; included after sushi_internal.hpp, track_margin_core.hpp and path_device.hpp.
#ifndef SUSHI_TRACK_MARGIN_DEVICE_HPP
#define SUSHI_TRACK_MARGIN_DEVICE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_margin_core.hpp"
#include "path_device.hpp"

namespace sushi {

// one set of partial records: entry b is workgroup b's
struct MarginPartials {
    double* c_min; double* m_min; double* a_min;
    int32_t* c_arg; int32_t* m_arg; int32_t* a_arg;
};

inline MarginPartials margin_set(char* mem, const MarginLayout& l, int set) {
    char* base = mem + (size_t)set * l.set_bytes;
    MarginPartials p;
    p.c_min = (double*)(base + l.c_min); p.m_min = (double*)(base + l.m_min); p.a_min = (double*)(base + l.a_min);
    p.c_arg = (int32_t*)(base + l.c_arg); p.m_arg = (int32_t*)(base + l.m_arg); p.a_arg = (int32_t*)(base + l.a_arg);
    return p;
}

// one of a record set's three first minima over all its records: every thread of the workgroup
__device__ __forceinline__ MinD reduce_records(const double* v, const int32_t* i, int n, PathLds& s) {
    // reduce_partials' pattern: a thread takes the records t, t + 256, ..., those past the end moved onto the last one -- every load
    // is always made, and all are in flight together; a record met twice changes nothing
    constexpr int ROUNDS = (int)(AXIS_MAX_GRID / TRACK_THREADS);
    int at[ROUNDS];
    double dv[ROUNDS];
    int32_t di[ROUNDS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) { const int r = (int)threadIdx.x + k * TRACK_THREADS; at[k] = r < n ? r : n - 1; }
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) { dv[k] = v[at[k]]; di[k] = i[at[k]]; }
    MinD m = {INFINITY, PATH_NO_INDEX};
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const bool take = path_min_replaces(dv[k], di[k], m.v, m.i);
        m.v = take ? dv[k] : m.v; m.i = take ? di[k] : m.i;
    }
    return block_first_min(m, s);
}

// The partial records of row `row` -> n_row, the minimum of C (every thread).  with_outputs (workgroup-uniform): the two minima of
// M are reduced as well, and thread 0 stores the row's outputs (Args: a launch's arguments -- `in`, n_partials, n_shift and c_min,
// best, best_arg, alt, alt_arg of the whole sequence).
template <typename Args>
__device__ __forceinline__ double reduce_margin_partials(const Args& a, bool with_outputs, int row, PathLds& s) {
    const MinD c = reduce_records(a.in.c_min, a.in.c_arg, a.n_partials, s);
    if (with_outputs) {
        const MinD m = reduce_records(a.in.m_min, a.in.m_arg, a.n_partials, s);
        const MinD o = reduce_records(a.in.a_min, a.in.a_arg, a.n_partials, s);
        if (threadIdx.x == 0) {
            a.c_min[row] = c.v;
            a.best[row] = m.v;
            a.best_arg[row] = path_clamp(m.i, a.n_shift);
            a.alt[row] = o.i == PATH_NO_INDEX ? INFINITY : o.v;
            a.alt_arg[row] = margin_alt_index(o.i, a.n_shift);
        }
    }
    return c.v;
}

}  // namespace sushi
#endif
