// sushi_amd/csrc/pcm_core.hpp -- the sample rule of sushi_hip_load_decode_format / _decode_mix_format (include/sushi_hip.h "sample
// formats"), one sample and one frame at a time.  Plain C++: sushi_pcm.hip runs it on the device,
// tests/host_pcm_check.cpp on the CPU (g++).  Both are compiled with -ffp-contract=off: every product and every sum rounds
// separately, as NumPy's float32 `*` and `+` do (sushi_amd.downmix.samples_from_bytes, mean_host, mix_host).
//
// A sample's value is a float32 on the int16 scale the rest of the load pipeline works on:
//   U8              (float)(((int)b - 128) * 256)
//   S16 / S24 / S32 the top two bytes of the container as int16 (downmix_core.hpp's downmix_sample: today's 24-bit rule, continued)
//   F32             s = v * 32768.0f, one float32 multiply; a NaN or +-inf s becomes +0.0f; denormals and -0.0f are values like any other
//   F64             s = (float)(v * 32768.0): a float64 multiply, one rounding to float32 (nearest-even); a NaN or +-inf s becomes +0.0f
// Nothing is clamped.  Every read is a byte read inside the sample's own container: a frame may lie at any address.
#ifndef SUSHI_PCM_CORE_HPP
#define SUSHI_PCM_CORE_HPP

#include <stdint.h>

#include "downmix_core.hpp"

namespace sushi {

// SUSHI_HIP_PCM_*
constexpr int PCM_U8 = 1, PCM_S16 = 2, PCM_S24 = 3, PCM_S32 = 4, PCM_F32 = 5, PCM_F64 = 6;

// container bytes of a sample; 0: no such format
DOWNMIX_HD constexpr int pcm_width(int format) {
    return format == PCM_U8 ? 1 : format == PCM_S16 ? 2 : format == PCM_S24 ? 3 : format == PCM_S32 || format == PCM_F32 ? 4 :
           format == PCM_F64 ? 8 : 0;
}

// s, or +0.0f where s is a NaN or an infinity (exponent bits all ones)
DOWNMIX_HD inline float pcm_finite_or_zero(float s) {
    uint32_t bits;
    __builtin_memcpy(&bits, &s, 4);
    return (bits & 0x7f800000u) == 0x7f800000u ? 0.0f : s;
}

// The sample whose container starts at p.
template <int FMT>
DOWNMIX_HD inline float pcm_sample(const uint8_t* p) {
    if constexpr (FMT == PCM_U8) {
        return (float)(((int)p[0] - 128) * 256);
    } else if constexpr (FMT == PCM_F32) {
        const uint32_t bits = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        float v;
        __builtin_memcpy(&v, &bits, 4);
        return pcm_finite_or_zero(v * 32768.0f);
    } else if constexpr (FMT == PCM_F64) {
        const uint32_t lo = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        const uint32_t hi = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
        const uint64_t bits = (uint64_t)lo | ((uint64_t)hi << 32);
        double v;
        __builtin_memcpy(&v, &bits, 8);
        const double scaled = v * 32768.0;
        return pcm_finite_or_zero((float)scaled);
    } else {
        static_assert(FMT == PCM_S16 || FMT == PCM_S24 || FMT == PCM_S32, "unknown sample format");
        return downmix_sample<pcm_width(FMT)>(p, 0);
    }
}

// The channel mean of one frame (wav.py:78-91 on the values above): the float32 sum left to right, divided by float(channels) --
// one channel: no division.
template <int FMT>
DOWNMIX_HD inline float pcm_mean(const uint8_t* frame, int channels) {
    constexpr int W = pcm_width(FMT);
    float acc = pcm_sample<FMT>(frame);
    for (int c = 1; c < channels; ++c) acc += pcm_sample<FMT>(frame + c * W);
    if (channels > 1) acc /= (float)channels;
    return acc;
}

// One (frame, output) of the weighted mix: downmix_value's statement on the values above.  Channel c's weight is w[c * stride].
template <int FMT>
DOWNMIX_HD inline float pcm_mix_value(const uint8_t* frame, int channels, const float* w, int stride) {
    constexpr int W = pcm_width(FMT);
    float acc = w[0] * pcm_sample<FMT>(frame);
    for (int c = 1; c < channels; ++c) {
        const float p = w[c * stride] * pcm_sample<FMT>(frame + c * W);
        acc = acc + p;
    }
    return acc;
}

// Every output of one frame with each sample read once: downmix_frame's order (the channel loop outermost, all
// DOWNMIX_MAX_OUTPUTS sums formed, w[c * DOWNMIX_MAX_OUTPUTS + o]) on the values above.
template <int FMT>
DOWNMIX_HD inline void pcm_mix_frame(const uint8_t* frame, int channels, const float* w, float (&acc)[DOWNMIX_MAX_OUTPUTS]) {
    constexpr int W = pcm_width(FMT);
    const float s0 = pcm_sample<FMT>(frame);
#pragma unroll
    for (int o = 0; o < DOWNMIX_MAX_OUTPUTS; ++o) acc[o] = w[o] * s0;
    for (int c = 1; c < channels; ++c) {
        const float s = pcm_sample<FMT>(frame + c * W);
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
