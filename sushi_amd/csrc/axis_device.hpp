// sushi_amd/csrc/axis_device.hpp -- the device side of the shift-axis layer (axis_core.hpp): how an extremum leaves a wave.  Shared
// by the reductions whose extrema travel as 64-bit (score, index) keys through atomicMin: the joint search (sushi_joint.hip) and the
// drift search (sushi_drift.hip).  Device code only; included after sushi_internal.hpp (the keys: sushi_common.hpp).
#ifndef SUSHI_AXIS_DEVICE_HPP
#define SUSHI_AXIS_DEVICE_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sushi_internal.hpp"
#include "axis_core.hpp"

namespace sushi {

template <bool MAX>
__device__ __forceinline__ unsigned long long joint_key(float v, unsigned pos) { return MAX ? make_key_max(v, pos) : make_key(v, pos); }

// A wave's smallest key into *slot.  Keys only ever fall, so a wave whose key is not below what the slot already holds has nothing to
// add: most waves leave after the load.
__device__ __forceinline__ void wave_key_min(unsigned long long key, unsigned long long* slot) {
    key = wave_min_u64(key);
    if ((threadIdx.x & 63) == 0 && key != NO_KEY &&
        key < __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(slot, key);
}

// the thread's own first extremum of one row's PER values (ascending index), as a key
template <int PER, bool MAX>
__device__ __forceinline__ unsigned long long thread_key(const float (&v)[PER], int64_t j0, int32_t n_shift) {
    constexpr int method = MAX ? SUSHI_HIP_METHOD_CCOEFF_NORMED : SUSHI_HIP_METHOD_SQDIFF_NORMED;
    if (j0 >= n_shift) return NO_KEY;
    float best = v[0];
    int64_t at = j0;
#pragma unroll
    for (int p = 1; p < PER; ++p) {
        const int64_t j = j0 + p * AXIS_THREADS;
        if (j < n_shift && axis_better(method, v[p], best)) { best = v[p]; at = j; }
    }
    return joint_key<MAX>(best, (unsigned)at);
}

}  // namespace sushi
#endif
