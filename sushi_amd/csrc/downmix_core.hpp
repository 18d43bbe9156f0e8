// sushi_amd/csrc/downmix_core.hpp -- the arithmetic of sushi_hip_load_decode_mix (include/sushi_hip.h "weighted downmix"; DESIGN.md
// 3.13), one frame at a time.  Plain C++: sushi_load.hip runs it on the device, tests/host_downmix_check.cpp on the CPU (g++).  Both
// are compiled with -ffp-contract=off: the product and the sum of every channel round separately, as NumPy's float32 `*` and `+` do.
#ifndef SUSHI_DOWNMIX_CORE_HPP
#define SUSHI_DOWNMIX_CORE_HPP

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DOWNMIX_HD __host__ __device__
#else
#define DOWNMIX_HD
#endif

namespace sushi {

constexpr int DOWNMIX_MAX_CHANNELS = 32;     // SUSHI_HIP_MIX_MAX_CHANNELS
constexpr int DOWNMIX_MAX_OUTPUTS = 8;       // SUSHI_HIP_MIX_MAX_OUTPUTS

// Channel c of the frame at `frame` (WIDTH bytes a sample, little endian) as wav.py:64-74 takes it: the int16 value (24-bit
// samples: their top two bytes) as float32.  Byte reads: a frame may lie at any address.
template <int WIDTH>
DOWNMIX_HD inline float downmix_sample(const uint8_t* frame, int c) {
    const uint8_t* p = frame + c * WIDTH + (WIDTH - 2);
    return (float)(int16_t)((uint16_t)p[0] | ((uint16_t)p[1] << 8));
}

// One (frame, output): acc = w[0] * s_0, then acc = acc + w[c] * s_c for c = 1 .. channels - 1 -- every channel in file order,
// zero weights included; each product and each sum is rounded to float32.  Channel c's weight is w[c * stride].
template <int WIDTH>
DOWNMIX_HD inline float downmix_value(const uint8_t* frame, int channels, const float* w, int stride) {
    float acc = w[0] * downmix_sample<WIDTH>(frame, 0);
    for (int c = 1; c < channels; ++c) {
        const float p = w[c * stride] * downmix_sample<WIDTH>(frame, c);
        acc = acc + p;
    }
    return acc;
}

// Every output of one frame with each sample read once: the operations of downmix_value per output, the channel loop outermost.
// w[c * DOWNMIX_MAX_OUTPUTS + o] is channel c's weight in output o.  All DOWNMIX_MAX_OUTPUTS sums are formed whatever the number of
// rows in use -- the weights of the others are zero and their sums are dropped: one eight-word load of uniform weights per
// channel and no branch in the loop.
template <int WIDTH>
DOWNMIX_HD inline void downmix_frame(const uint8_t* frame, int channels, const float* w, float (&acc)[DOWNMIX_MAX_OUTPUTS]) {
    const float s0 = downmix_sample<WIDTH>(frame, 0);
#pragma unroll
    for (int o = 0; o < DOWNMIX_MAX_OUTPUTS; ++o) acc[o] = w[o] * s0;
    for (int c = 1; c < channels; ++c) {
        const float s = downmix_sample<WIDTH>(frame, c);
        const float* wc = w + c * DOWNMIX_MAX_OUTPUTS;
#pragma unroll
        for (int o = 0; o < DOWNMIX_MAX_OUTPUTS; ++o) {
            const float p = wc[o] * s;
            acc[o] = acc[o] + p;
        }
    }
}

}  // namespace sushi
#endif
