// sushi_amd/csrc/sushi_pcm.hip -- the load pipeline's decode for every sample format a WAV file carries (gfx950): 8-bit, 16-,
// 24- and 32-bit integer, 32- and 64-bit float (include/sushi_hip.h "sample formats").
//
// sushi_hip_load_decode_format / sushi_hip_load_decode_mix_format are sushi_hip_load_decode / sushi_hip_load_decode_mix
// (sushi_load.hip) with a format code in place of the sample width: the same mean, the same weighted mix, on the values pcm_core.hpp
// gives a sample.  Compiled with -ffp-contract=off: every product and every sum rounds separately, so the NumPy restatement
// (sushi_amd.downmix.samples_from_bytes, mean_host, mix_host) equals the result bit for bit.
//
// Both kernels are single passes: the file's bytes in, 4 B out per frame and row.  Byte loads, so the PCM may lie at any address;
// a wave's 64 threads read 64 consecutive frames = one contiguous run of bytes, which the caches turn into whole lines.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "pcm_core.hpp"

namespace {

using sushi::launch_ok;

static_assert(sushi::PCM_U8 == SUSHI_HIP_PCM_U8 && sushi::PCM_S16 == SUSHI_HIP_PCM_S16 && sushi::PCM_S24 == SUSHI_HIP_PCM_S24 &&
              sushi::PCM_S32 == SUSHI_HIP_PCM_S32 && sushi::PCM_F32 == SUSHI_HIP_PCM_F32 && sushi::PCM_F64 == SUSHI_HIP_PCM_F64,
              "pcm_core.hpp's codes are the header's");

constexpr int TILE = 256;         // frames per workgroup: one per thread
constexpr int64_t MAX_GRID = 65536;   // workgroups of a launch; longer runs of frames go round the grid-stride loop

// One thread per frame: the channel mean of the frame's samples (pcm_core.hpp pcm_mean).  Offsets are 64-bit.
template <int FMT>
__global__ __launch_bounds__(TILE)
void decode_format_kernel(const uint8_t* __restrict__ pcm, int64_t n_frames, int channels, float* __restrict__ mono) {
    const int64_t fs = (int64_t)channels * sushi::pcm_width(FMT);
    for (int64_t f = (int64_t)blockIdx.x * TILE + threadIdx.x; f < n_frames; f += (int64_t)gridDim.x * TILE)
        mono[f] = sushi::pcm_mean<FMT>(pcm + f * fs, channels);
}

// The weights travel in the kernel's arguments (w[c * 8 + o], wave-uniform: scalar loads), as sushi_load.hip's MixArgs.
struct PcmMixArgs {
    const uint8_t* pcm;     // any byte alignment
    int64_t n_frames;
    float* out;             // row o: out + o * out_stride
    int64_t out_stride;
    int32_t channels, n_out;
    float w[sushi::DOWNMIX_MAX_CHANNELS * sushi::DOWNMIX_MAX_OUTPUTS];
};
static_assert(sizeof(PcmMixArgs) <= 1280, "PcmMixArgs travels as kernel arguments");

// One thread per frame: all eight sums of the frame (pcm_core.hpp pcm_mix_frame; acc[] is indexed by unrolled loops only: registers),
// the rows in use stored as n_out runs of 64 consecutive floats per wave.
template <int FMT>
__global__ __launch_bounds__(TILE)
void decode_mix_format_kernel(PcmMixArgs a) {
    const int64_t fs = (int64_t)a.channels * sushi::pcm_width(FMT);
    for (int64_t f = (int64_t)blockIdx.x * TILE + threadIdx.x; f < a.n_frames; f += (int64_t)gridDim.x * TILE) {
        float acc[sushi::DOWNMIX_MAX_OUTPUTS];
        sushi::pcm_mix_frame<FMT>(a.pcm + f * fs, a.channels, a.w, acc);
#pragma unroll
        for (int k = 0; k < sushi::DOWNMIX_MAX_OUTPUTS; ++k)
            if (k < a.n_out) a.out[k * a.out_stride + f] = acc[k];
    }
}

inline unsigned grid_for(int64_t n_frames) {
    const int64_t want = (n_frames + TILE - 1) / TILE;
    return (unsigned)(want < MAX_GRID ? want : MAX_GRID);
}

template <int FMT>
void launch_decode(const uint8_t* pcm, int64_t n_frames, int channels, float* mono, hipStream_t st) {
    hipLaunchKernelGGL(decode_format_kernel<FMT>, dim3(grid_for(n_frames)), dim3(TILE), 0, st, pcm, n_frames, channels, mono);
}

template <int FMT>
void launch_mix(const PcmMixArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(decode_mix_format_kernel<FMT>, dim3(grid_for(a.n_frames)), dim3(TILE), 0, st, a);
}

}  // namespace

extern "C" {

int sushi_hip_load_decode_format(const void* pcm_dev, int64_t n_frames, int32_t channels, int32_t format, float* mono_dev,
                                 void* hip_stream) {
    if (!pcm_dev || !mono_dev || n_frames < 0 || channels < 1) return SUSHI_HIP_EINVAL;
    if (sushi::pcm_width(format) == 0) return SUSHI_HIP_EINVAL;
    if ((uintptr_t)mono_dev & 3) return SUSHI_HIP_EALIGN;
    if (n_frames == 0) return SUSHI_HIP_OK;
    const uint8_t* pcm = (const uint8_t*)pcm_dev;
    hipStream_t st = (hipStream_t)hip_stream;
    switch (format) {
        case SUSHI_HIP_PCM_U8: launch_decode<sushi::PCM_U8>(pcm, n_frames, channels, mono_dev, st); break;
        case SUSHI_HIP_PCM_S16: launch_decode<sushi::PCM_S16>(pcm, n_frames, channels, mono_dev, st); break;
        case SUSHI_HIP_PCM_S24: launch_decode<sushi::PCM_S24>(pcm, n_frames, channels, mono_dev, st); break;
        case SUSHI_HIP_PCM_S32: launch_decode<sushi::PCM_S32>(pcm, n_frames, channels, mono_dev, st); break;
        case SUSHI_HIP_PCM_F32: launch_decode<sushi::PCM_F32>(pcm, n_frames, channels, mono_dev, st); break;
        default: launch_decode<sushi::PCM_F64>(pcm, n_frames, channels, mono_dev, st); break;
    }
    return launch_ok();
}

int sushi_hip_load_decode_mix_format(const void* pcm_dev, int64_t n_frames, int32_t channels, int32_t format,
                                     const float* weights_host, int32_t n_out, float* out_dev, int64_t out_stride,
                                     void* hip_stream) {
    if (!pcm_dev || !weights_host || !out_dev || n_frames < 0) return SUSHI_HIP_EINVAL;
    if (channels < 1 || channels > SUSHI_HIP_MIX_MAX_CHANNELS || n_out < 1 || n_out > SUSHI_HIP_MIX_MAX_OUTPUTS) return SUSHI_HIP_EINVAL;
    if (sushi::pcm_width(format) == 0) return SUSHI_HIP_EINVAL;
    if (out_stride < n_frames) return SUSHI_HIP_EINVAL;
    for (int k = 0; k < n_out * channels; ++k)
        if (!std::isfinite(weights_host[k])) return SUSHI_HIP_EINVAL;
    if ((uintptr_t)out_dev & 3) return SUSHI_HIP_EALIGN;
    if (n_frames == 0) return SUSHI_HIP_OK;
    PcmMixArgs a;
    a.pcm = (const uint8_t*)pcm_dev; a.n_frames = n_frames; a.out = out_dev; a.out_stride = out_stride;
    a.channels = channels; a.n_out = n_out;
    for (int c = 0; c < sushi::DOWNMIX_MAX_CHANNELS; ++c)
        for (int o = 0; o < sushi::DOWNMIX_MAX_OUTPUTS; ++o)
            a.w[c * sushi::DOWNMIX_MAX_OUTPUTS + o] = c < channels && o < n_out ? weights_host[o * channels + c] : 0.f;
    hipStream_t st = (hipStream_t)hip_stream;
    switch (format) {
        case SUSHI_HIP_PCM_U8: launch_mix<sushi::PCM_U8>(a, st); break;
        case SUSHI_HIP_PCM_S16: launch_mix<sushi::PCM_S16>(a, st); break;
        case SUSHI_HIP_PCM_S24: launch_mix<sushi::PCM_S24>(a, st); break;
        case SUSHI_HIP_PCM_S32: launch_mix<sushi::PCM_S32>(a, st); break;
        case SUSHI_HIP_PCM_F32: launch_mix<sushi::PCM_F32>(a, st); break;
        default: launch_mix<sushi::PCM_F64>(a, st); break;
    }
    return launch_ok();
}

}  // extern "C"
