// sushi_amd/csrc/envelope_core.hpp -- the arithmetic of sushi_hip_envelope (include/sushi_hip.h "loudness contour"):
// the mean absolute deviation about the sample type's nominal centre over span blocks of hop samples, one output per block.
// Plain C++: sushi_envelope.hip runs it on the device, tests/host_envelope_check.cpp on the CPU (g++).  Both are compiled with
// -ffp-contract=off, and every float64 sum is sequential in a stated order: each addition rounds once, as NumPy's do.
// Behind it, host only: stage_envelope -- the arguments of a call -> a refusal, or the tile, the tile count and the grid.
#ifndef SUSHI_ENVELOPE_CORE_HPP
#define SUSHI_ENVELOPE_CORE_HPP

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/sushi_hip.h"
#include "row_core.hpp"            // row_at, row_deviation, row_call_ok

namespace sushi {

constexpr int32_t ENVELOPE_MAX_HOP = 256;
constexpr int32_t ENVELOPE_MAX_SPAN = 64;
constexpr int32_t ENVELOPE_MAX_WINDOW = 4096;                  // hop * span

// What a sum of deviations is kept in: float64 for float32 samples, an integer for uint8 (at most 4096 * 128 = 524288).
template <class T> struct EnvelopeSum;
template <> struct EnvelopeSum<float> { typedef double type; };
template <> struct EnvelopeSum<uint8_t> { typedef uint32_t type; };

// |x - c|, c = sushi_hip_centre: 0.5 (the difference rounds once, in float64) or 128 (stated in unsigned integers here: through
// row_deviation's signed difference the uint8 kernel compiles to other code).
SUSHI_GEOM_HD inline double envelope_deviation(float x) { return fabs(row_deviation(x)); }
SUSHI_GEOM_HD inline uint32_t envelope_deviation(uint8_t x) { return x >= 128 ? (uint32_t)x - 128u : 128u - (uint32_t)x; }

// Blocks in front of output i: a = (span - 1) / 2; output i sums blocks i - a .. i - a + span - 1.
SUSHI_GEOM_HD inline int32_t envelope_lead(int32_t span) { return (span - 1) / 2; }

// A block sum B: sample(t), t = 0 .. hop - 1, in that order (sample: where the block's samples are -- the row with both clamps
// on the CPU, the staged tile on the device).
template <class T, class Sample>
SUSHI_GEOM_HD inline typename EnvelopeSum<T>::type envelope_block(Sample sample, int32_t hop) {
    typename EnvelopeSum<T>::type acc = 0;
    int32_t t = 0;
    for (; t + 8 <= hop; t += 8) {                          // eight reads in flight, the additions in order all the same
        T v[8];
        for (int k = 0; k < 8; ++k) v[k] = (T)sample(t + k);
        for (int k = 0; k < 8; ++k) acc = acc + envelope_deviation(v[k]);
    }
    for (; t < hop; ++t) acc = acc + envelope_deviation((T)sample(t));
    return acc;
}

// E of an output: block(j), j = 0 .. span - 1, in that order.
template <class T, class Block>
SUSHI_GEOM_HD inline typename EnvelopeSum<T>::type envelope_window(Block block, int32_t span) {
    typename EnvelopeSum<T>::type acc = 0;
    for (int32_t j = 0; j < span; ++j) acc = acc + block(j);
    return acc;
}

// E -> the output sample: 2 E / W, W = hop * span.  float32: (float)((E + E) / (double)W); uint8: rounded half up in integers
// (4 E + W <= 2^21 + 2^12), capped at 255 (a row of 0 gives 256).
SUSHI_GEOM_HD inline float envelope_finish(double e, int32_t w, const float*) { return (float)((e + e) / (double)w); }
SUSHI_GEOM_HD inline uint8_t envelope_finish(uint32_t e, int32_t w, const uint8_t*) {
    const uint32_t y = (4u * e + (uint32_t)w) / (2u * (uint32_t)w);
    return (uint8_t)(y < 255u ? y : 255u);
}

// One output straight from the row (the CPU check; the kernel forms the same sums, in the same order, from its staged tile).
template <class T>
inline T envelope_sample(const T* x, int64_t n_in, int64_t in_start, int32_t hop, int32_t span, int64_t i) {
    typedef typename EnvelopeSum<T>::type S;
    const int64_t b0 = i - envelope_lead(span);
    const S e = envelope_window<T>([&](int32_t j) {
        const int64_t g0 = in_start + (b0 + j) * hop;
        return envelope_block<T>([&](int32_t t) { return row_at(x, n_in, g0 + t); }, hop);
    }, span);
    return envelope_finish(e, hop * span, (const T*)0);
}

// ---- the tile of a workgroup ----
// ENVELOPE_THREADS threads own `tile` consecutive outputs: tile * hop is at most ENVELOPE_TILE_SAMPLES, tile at most
// ENVELOPE_MAX_TILE (hop <= 8) and at least 16 (hop 256).  They stage the samples of the tile's blocks, tile + span - 1 of them,
// one 32-bit word per sample, a block's words `stride` apart: the odd number hop | 1, so that threads that walk neighbouring
// blocks in step read different LDS banks.
constexpr int ENVELOPE_THREADS = 256;
constexpr int32_t ENVELOPE_TILE_SAMPLES = 4096;
constexpr int32_t ENVELOPE_MAX_TILE = 512;
constexpr int64_t ENVELOPE_MAX_GRID = 1024;                    // a fixed grid striding over the tiles: 256 CUs, four workgroups each (what LDS lets a CU hold)

SUSHI_GEOM_HD constexpr int32_t envelope_tile(int32_t hop) {
    return ENVELOPE_TILE_SAMPLES / hop < ENVELOPE_MAX_TILE ? ENVELOPE_TILE_SAMPLES / hop : ENVELOPE_MAX_TILE;
}
SUSHI_GEOM_HD constexpr int32_t envelope_stride(int32_t hop) { return hop | 1; }
SUSHI_GEOM_HD constexpr int32_t envelope_max_span(int32_t hop) {
    return ENVELOPE_MAX_WINDOW / hop < ENVELOPE_MAX_SPAN ? ENVELOPE_MAX_WINDOW / hop : ENVELOPE_MAX_SPAN;
}
// the most words / block sums a tile stages, over every hop and the widest span it allows
constexpr int32_t envelope_max_blocks() {
    int32_t most = 0;
    for (int32_t h = 1; h <= ENVELOPE_MAX_HOP; ++h) {
        const int32_t nb = envelope_tile(h) + envelope_max_span(h) - 1;
        most = nb > most ? nb : most;
    }
    return most;
}
constexpr int32_t envelope_max_words() {
    int32_t most = 0;
    for (int32_t h = 1; h <= ENVELOPE_MAX_HOP; ++h) {
        const int32_t words = (envelope_tile(h) + envelope_max_span(h) - 1) * envelope_stride(h);
        most = words > most ? words : most;
    }
    return most;
}
constexpr int32_t ENVELOPE_STAGE_WORDS = envelope_max_words();
constexpr int32_t ENVELOPE_STAGE_BLOCKS = envelope_max_blocks();
static_assert((ENVELOPE_STAGE_WORDS + 1) * 4 + ENVELOPE_STAGE_BLOCKS * 8 <= 40 * 1024, "a tile's samples and block sums fit 40 KB of LDS: four workgroups to a CU");

// ---- the host side of a call ----
struct EnvelopeStage {
    int32_t tile;             // outputs per tile
    int64_t n_tiles;
    unsigned grid;
};

// EINVAL: an unknown dtype, n_in < 1 (or >= 2^62), out_len outside 1 .. 2^40 - 1, in_start outside [0, n_in - 1], hop outside
// 1 .. 256, span outside 1 .. 64, hop * span > 4096 (`out` is then unspecified).
inline int stage_envelope(int dtype, int64_t n_in, int64_t in_start, int32_t hop, int32_t span, int64_t out_len, EnvelopeStage& out) {
    if (row_call_ok(dtype, n_in, in_start, out_len) != SUSHI_HIP_OK) return SUSHI_HIP_EINVAL;
    if (hop < 1 || hop > ENVELOPE_MAX_HOP || span < 1 || span > ENVELOPE_MAX_SPAN || hop * span > ENVELOPE_MAX_WINDOW) return SUSHI_HIP_EINVAL;
    out.tile = envelope_tile(hop);
    out.n_tiles = (out_len + out.tile - 1) / out.tile;
    out.grid = (unsigned)(out.n_tiles < ENVELOPE_MAX_GRID ? out.n_tiles : ENVELOPE_MAX_GRID);
    return SUSHI_HIP_OK;
}

}  // namespace sushi
#endif
