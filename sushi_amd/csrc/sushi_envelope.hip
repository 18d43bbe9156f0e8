// sushi_amd/csrc/sushi_envelope.hip -- sushi_hip_envelope: a row's loudness contour (gfx950).
//
// Output i is the mean absolute deviation about the sample type's centre over span blocks of hop samples, in the arithmetic
// include/sushi_hip.h states and envelope_core.hpp implements (float32: float64 sums, sequential in a stated order; this unit is
// compiled with -ffp-contract=off), so that the output is bit-identical to the NumPy restatement (sushi_amd/envelope.py
// envelope_host).
//
// A workgroup of 256 threads owns a tile of consecutive outputs (envelope_tile(hop): about 4096 input samples' worth, at most 512
// outputs) and strides over the tiles on a fixed grid.  Per tile:
//   1. the samples of the tile's tile + span - 1 blocks come into LDS with 16-byte loads on the grid of 16-byte-aligned ADDRESSES
//      (the first vector starts up to 15 bytes in front of the tile's first sample; in_start has only sample alignment); a tile
//      whose vectors cross either end of the row is read sample by sample with the clamp instead (one branch per workgroup).
//      A sample is one 32-bit LDS word, a block's words hop | 1 apart: threads that walk neighbouring blocks in step read
//      different banks.
//   2. a thread forms a block's sum from LDS, sequentially in t, and leaves it in LDS;
//   3. a thread sums span of them in order, finishes and stores its output (out_dev has only sample alignment: plain stores of
//      consecutive samples by consecutive lanes).
// No atomics, no workspace.  uint8 samples take the same path with integer sums: per input byte it is bound by the LDS pass, not
// by memory (profiles/envelope/README.md).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "envelope_core.hpp"

namespace {

using namespace sushi;

struct EnvelopeArgs {
    const void* in;
    int64_t n_in, in_start;
    int32_t hop, span, tile;
    int64_t n_tiles;
    void* out;
    int64_t out_len;
};

// a sample as its LDS word, and back
__device__ inline uint32_t to_word(float v) { return __float_as_uint(v); }
__device__ inline uint32_t to_word(uint8_t v) { return v; }
// sample k of a 16-byte vector's four dwords, as its LDS word
__device__ inline uint32_t word_of(const uint32_t (&dw)[4], int k, const float*) { return dw[k]; }
__device__ inline uint32_t word_of(const uint32_t (&dw)[4], int k, const uint8_t*) { return (dw[k >> 2] >> (8 * (k & 3))) & 0xffu; }
__device__ inline float from_word(uint32_t w, const float*) { return __uint_as_float(w); }
__device__ inline uint8_t from_word(uint32_t w, const uint8_t*) { return (uint8_t)w; }

template <class T>
__global__ __launch_bounds__(ENVELOPE_THREADS)
void envelope_kernel(EnvelopeArgs a) {
    typedef typename EnvelopeSum<T>::type S;
    constexpr int PER = 16 / (int)sizeof(T);                // samples of a 16-byte vector
    constexpr int LOADS = 4;                                // vectors a thread has in flight (a float32 tile is up to 9 a thread)
    __shared__ uint32_t stage[ENVELOPE_STAGE_WORDS + 1];    // (+ a spare word: where a vector's samples outside the tile go)
    __shared__ S sums[ENVELOPE_STAGE_BLOCKS];
    const T* __restrict__ x = (const T*)a.in;
    T* __restrict__ out = (T*)a.out;
    const int32_t hop = a.hop, span = a.span, stride = envelope_stride(hop);
    const uint32_t skip = (uint32_t)(stride - hop);        // words between a block's last sample and the next block's first
    const int tid = threadIdx.x;
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t i0 = tile * a.tile;
        const int32_t n_out = (int32_t)(a.out_len - i0 < a.tile ? a.out_len - i0 : a.tile);
        const int32_t n_blocks = n_out + span - 1;
        const int32_t n_samples = n_blocks * hop;           // <= ENVELOPE_TILE_SAMPLES + ENVELOPE_MAX_WINDOW
        const int64_t g0 = a.in_start + (i0 - envelope_lead(span)) * hop;     // the tile's first sample (may lie outside the row)
        // 1. stage: vector v holds samples first + v * PER ..., `first` on the address grid at or in front of g0
        const int32_t phase = (int32_t)((((uintptr_t)x + (uintptr_t)(g0 * (int64_t)sizeof(T))) & 15) / sizeof(T));
        const int64_t first = g0 - phase;
        const int32_t n_vec = (n_samples + phase + PER - 1) / PER;
        if (first >= 0 && first + (int64_t)n_vec * PER <= a.n_in) {       // (the same for the whole workgroup) every vector lies inside the row
            const uint4* __restrict__ xv = reinterpret_cast<const uint4*>(x + first);         // 16-byte aligned: `first` lies on the address grid
            // LOADS vectors a thread at a time: their loads are all out before the first is consumed
            for (int32_t v0 = tid; v0 < n_vec; v0 += LOADS * ENVELOPE_THREADS) {
                uint4 pk[LOADS];
#pragma unroll
                for (int u = 0; u < LOADS; ++u)
                    if (v0 + u * ENVELOPE_THREADS < n_vec) pk[u] = xv[v0 + u * ENVELOPE_THREADS];
#pragma unroll
                for (int u = 0; u < LOADS; ++u) {
                    const int32_t v = v0 + u * ENVELOPE_THREADS;
                    if (v >= n_vec) break;
                    const uint32_t dw[4] = {pk[u].x, pk[u].y, pk[u].z, pk[u].w};
                    const int32_t s0 = v * PER - phase;      // the vector's first sample, counted from the tile's first
                    const int32_t k0 = s0 < 0 ? -s0 : 0;     // (only vector 0 starts in front of it)
                    const uint32_t sb = (uint32_t)(s0 + k0);
                    const uint32_t q = sb / (uint32_t)hop;
                    uint32_t r = sb - q * (uint32_t)hop;
                    uint32_t w = q * (uint32_t)stride + r;
                    // no branch per sample: one outside the tile goes to the spare word, and only a sample of the tile advances (w, r)
#pragma unroll
                    for (int k = 0; k < PER; ++k) {
                        const bool in_front = k < k0;
                        const bool valid = !in_front && s0 + k < n_samples;
                        stage[valid ? w : (uint32_t)ENVELOPE_STAGE_WORDS] = word_of(dw, k, (const T*)0);
                        const uint32_t step = in_front ? 0u : 1u;
                        w += step; r += step;
                        const bool wrap = r == (uint32_t)hop;
                        r = wrap ? 0u : r;
                        w += wrap ? skip : 0u;
                    }
                }
            }
        } else {                                             // a tile at either end of the row, or past it: sample by sample, with the clamp
            for (int32_t sm = tid; sm < n_samples; sm += ENVELOPE_THREADS) {
                const uint32_t q = (uint32_t)sm / (uint32_t)hop;
                stage[q * (uint32_t)stride + ((uint32_t)sm - q * (uint32_t)hop)] = to_word(row_at(x, a.n_in, g0 + sm));
            }
        }
        __syncthreads();
        // 2. block sums
        for (int32_t b = tid; b < n_blocks; b += ENVELOPE_THREADS) {
            const uint32_t* __restrict__ blk = stage + b * stride;
            sums[b] = envelope_block<T>([&](int32_t t) { return from_word(blk[t], (const T*)0); }, hop);
        }
        __syncthreads();
        // 3. outputs
        for (int32_t i = tid; i < n_out; i += ENVELOPE_THREADS) {
            const S e = envelope_window<T>([&](int32_t j) { return sums[i + j]; }, span);
            out[i0 + i] = envelope_finish(e, hop * span, (const T*)0);
        }
        __syncthreads();                                    // the next tile stages over what this one read
    }
}

}  // namespace

extern "C" {

int sushi_hip_envelope(const void* in_dev, int dtype, int64_t n_in, int64_t in_start, int32_t hop, int32_t span,
                       void* out_dev, int64_t out_len, void* hip_stream) { return c_boundary([&]() -> int {
    if (!in_dev || !out_dev) return SUSHI_HIP_EINVAL;
    EnvelopeStage staged;
    const int rc = stage_envelope(dtype, n_in, in_start, hop, span, out_len, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if (!row_aligned(in_dev, dtype) || !row_aligned(out_dev, dtype)) return SUSHI_HIP_EALIGN;

    hipStream_t st = (hipStream_t)hip_stream;
    EnvelopeArgs a;
    a.in = in_dev; a.n_in = n_in; a.in_start = in_start; a.hop = hop; a.span = span; a.tile = staged.tile; a.n_tiles = staged.n_tiles;
    a.out = out_dev; a.out_len = out_len;
    row_dispatch(dtype, [&](auto t) { hipLaunchKernelGGL(envelope_kernel<decltype(t)>, dim3(staged.grid), dim3(ENVELOPE_THREADS), 0, st, a); });
    return launch_ok();
}); }

}  // extern "C"
