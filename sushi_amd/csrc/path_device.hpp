// sushi_amd/csrc/path_device.hpp -- the device side the passes with one launch per row share: the segmentation pass
// (sushi_path.hip) and the tracking pass (sushi_track.hip).  How the minimum of D_e -- a float64 and an index: no 64-bit key --
// leaves a wave and a workgroup, and how it travels to the next launch: every workgroup leaves one partial record, and every
// workgroup of the next launch begins by reducing those records under a rule that does not depend on the order they meet in
// (path_core.hpp: the lower index wins a tie).  Device code only; included after sushi_internal.hpp and path_core.hpp.
#ifndef SUSHI_PATH_DEVICE_HPP
#define SUSHI_PATH_DEVICE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "path_core.hpp"

namespace sushi {

// one set of partial records: entry b is workgroup b's
struct PathPartials {
    double* d_min; int32_t* d_arg;          // the first minimum of D over the workgroup's items
    int32_t* own_idx; float* own_val;       // the row's own first extremum over them
};

enum { PREV_NONE = 0, PREV_PARTIALS = 1, PREV_ROW_MIN = 2 };

struct MinD { double v; int32_t i; };
struct OwnF { float v; int32_t i; };

__device__ __forceinline__ MinD wave_first_min(MinD a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double ov = __shfl_down(a.v, d, 64);
        const int32_t oi = __shfl_down(a.i, d, 64);
        if (path_min_replaces(ov, oi, a.v, a.i)) { a.v = ov; a.i = oi; }
    }
    return a;                               // valid in lane 0
}
template <int METHOD>
__device__ __forceinline__ OwnF wave_first_own(OwnF a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float ov = __shfl_down(a.v, d, 64);
        const int32_t oi = __shfl_down(a.i, d, 64);
        if (path_own_replaces(METHOD, ov, oi, a.v, a.i)) { a.v = ov; a.i = oi; }
    }
    return a;
}

// the four waves' results through a few words of LDS: valid in every thread.  Two barriers, the first of which also lets the last
// readers of an earlier call through: every thread of the workgroup calls it.
struct PathLds { double dv[4]; int32_t di[4]; float ov[4]; int32_t oi[4]; };
__device__ __forceinline__ MinD block_first_min(MinD a, PathLds& s) {
    a = wave_first_min(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s.dv[threadIdx.x >> 6] = a.v; s.di[threadIdx.x >> 6] = a.i; }
    __syncthreads();
    MinD m = {s.dv[0], s.di[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (path_min_replaces(s.dv[w], s.di[w], m.v, m.i)) { m.v = s.dv[w]; m.i = s.di[w]; }
    return m;
}
template <int METHOD>
__device__ __forceinline__ OwnF block_first_own(OwnF a, PathLds& s) {
    a = wave_first_own<METHOD>(a);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s.ov[threadIdx.x >> 6] = a.v; s.oi[threadIdx.x >> 6] = a.i; }
    __syncthreads();
    OwnF m = {s.ov[0], s.oi[0]};
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (path_own_replaces(METHOD, s.ov[w], s.oi[w], m.v, m.i)) { m.v = s.ov[w]; m.i = s.oi[w]; }
    return m;
}

template <int METHOD>
__device__ __forceinline__ float own_worst() { return METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED ? -INFINITY : INFINITY; }

// The partial records of one row -> its minimum (every thread of the workgroup).  with_outputs (workgroup-uniform): the row's own
// extremum is reduced as well, and thread 0 stores the row's four outputs (Args: a launch's arguments -- row_min, row_arg,
// row_own_index, row_own_score of the whole sequence, and n_shift).
template <int METHOD, typename Args>
__device__ __forceinline__ double reduce_partials(const PathPartials& in, int n, bool with_outputs, int row, const Args& a,
                                                  PathLds& s) {
    // a thread takes the records t, t + 256, ... (AXIS_MAX_GRID / PATH_THREADS of them), those past the end moved onto the last one --
    // every load is always made, and all are in flight together; a record met twice changes nothing
    constexpr int ROUNDS = (int)(AXIS_MAX_GRID / PATH_THREADS);
    int at[ROUNDS];
    double dv[ROUNDS];
    int32_t di[ROUNDS];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) { const int i = (int)threadIdx.x + k * PATH_THREADS; at[k] = i < n ? i : n - 1; }
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) { dv[k] = in.d_min[at[k]]; di[k] = in.d_arg[at[k]]; }
    MinD m = {INFINITY, PATH_NO_INDEX};
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const bool take = path_min_replaces(dv[k], di[k], m.v, m.i);
        m.v = take ? dv[k] : m.v; m.i = take ? di[k] : m.i;
    }
    m = block_first_min(m, s);
    if (with_outputs) {
        float ov[ROUNDS];
        int32_t oi[ROUNDS];
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) { ov[k] = in.own_val[at[k]]; oi[k] = in.own_idx[at[k]]; }
        OwnF o = {own_worst<METHOD>(), PATH_NO_INDEX};
#pragma unroll
        for (int k = 0; k < ROUNDS; ++k) {
            const bool take = path_own_replaces(METHOD, ov[k], oi[k], o.v, o.i);
            o.v = take ? ov[k] : o.v; o.i = take ? oi[k] : o.i;
        }
        o = block_first_own<METHOD>(o, s);
        if (threadIdx.x == 0) {
            a.row_min[row] = m.v;
            a.row_arg[row] = path_clamp(m.i, a.n_shift);
            a.row_own_index[row] = path_clamp(o.i, a.n_shift);
            a.row_own_score[row] = o.v;
        }
    }
    return m.v;
}

inline PathPartials partial_set(char* mem, const PathLayout& l, int set) {
    char* base = mem + (size_t)set * l.set_bytes;
    PathPartials p;
    p.d_min = (double*)(base + l.d_min); p.d_arg = (int32_t*)(base + l.d_arg);
    p.own_idx = (int32_t*)(base + l.own_idx); p.own_val = (float*)(base + l.own_val);
    return p;
}

}  // namespace sushi
#endif
