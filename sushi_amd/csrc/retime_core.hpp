// sushi_amd/csrc/retime_core.hpp -- the arithmetic of sushi_hip_retime (include/sushi_hip.h "retiming"), one sample
// at a time.  Plain C++: sushi_retime.hip runs it on the device, tests/host_retime_check.cpp on the CPU (g++).  Both are compiled
// with -ffp-contract=off: the product and the sum of the interpolation round separately, as NumPy's do.
// Behind it, host only: the segment record the kernel reads, and stage_retime -- segments -> a refusal, or the table that is uploaded
// and the facts of the launch (tests/host_stream_check.cpp states what a staged call must be).
#ifndef SUSHI_RETIME_CORE_HPP
#define SUSHI_RETIME_CORE_HPP

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/sushi_hip.h"
#include "sushi_geometry.hpp"      // align_up
#include "row_core.hpp"            // the sample type of a call, the cursor of a rational step

namespace sushi {

// Where output i of a segment reads its input: position in_start + i * num / den = sample j and the fraction r / den behind it.
// One division per run of outputs (row_core.hpp), then from output i to output i + 1 without another: r += num % den, the carry
// and num / den go into j.
typedef RowCursor RetimeCursor;
SUSHI_GEOM_HD inline RetimeCursor retime_seek(int64_t in_start, int64_t i, int32_t num, int32_t den) { return row_seek(in_start, i, num, den); }
SUSHI_GEOM_HD inline void retime_advance(RetimeCursor& c, int32_t qstep, int32_t rstep, int32_t den) { row_advance(c, qstep, rstep, den); }

SUSHI_GEOM_HD inline float retime_round(double y, const float*) { return (float)y; }
SUSHI_GEOM_HD inline uint8_t retime_round(double y, const uint8_t*) { return (uint8_t)(y + 0.5); }       // half up (y >= 0)

// One output sample (T: float or uint8_t): y = x[j] + w * (x[j1] - x[j]) in float64, w = r / den, j1 = min(j + 1, n_in - 1);
// float32: (float)y; uint8: (uint8_t)(y + 0.5).
template <class T>
SUSHI_GEOM_HD inline T retime_sample(const T* x, int64_t n_in, int64_t j, int32_t r, int32_t den) {
    const int64_t j1 = j + 1 < n_in - 1 ? j + 1 : n_in - 1;
    const double a = (double)x[j];
    const double b = (double)x[j1];
    const double w = (double)r / (double)den;
    const double d = b - a;
    const double p = w * d;
    const double y = a + p;
    return retime_round(y, (const T*)0);
}

// ---- the host side of a call ----
// a segment on the device
struct RetimeSeg {
    int64_t in_start, out_off, out_len;
    int64_t first_tile;       // tiles of the segments before this one
    int32_t num, den;
    int32_t phase;            // samples between the 16-byte boundary at or in front of the segment's first output and that output
    int32_t reserved;
};
static_assert(sizeof(RetimeSeg) == 48, "RetimeSeg layout");

// A segment's outputs are cut into chunks of PER consecutive samples, one per thread, RETIME_THREADS chunks to a tile.
template <class T> struct RetimeChunk;
template <> struct RetimeChunk<float> { static constexpr int PER = 8; };        // two 16-byte stores
template <> struct RetimeChunk<uint8_t> { static constexpr int PER = 16; };     // one
constexpr int RETIME_THREADS = 256;
constexpr int64_t RETIME_MAX_GRID = 2048;                // a fixed grid striding over the tiles: 256 CUs, eight workgroups each (a CU holds eight of these)

// workspace: the table
inline size_t retime_layout_bytes(int n_seg) { return n_seg < 1 ? 0 : align_up((size_t)n_seg * sizeof(RetimeSeg), 256); }

constexpr int32_t RETIME_MAX_TERM = 1 << 20;             // num, den

inline bool segment_ok(const SushiHipRetimeSegment& s, int64_t n_in, int64_t n_out) {
    if (s.num < 1 || s.num > RETIME_MAX_TERM || s.den < 1 || s.den > RETIME_MAX_TERM) return false;
    if ((int64_t)s.num > 8 * (int64_t)s.den || (int64_t)s.den > 8 * (int64_t)s.num) return false;
    if (s.out_len < 1 || s.out_len >= ROW_MAX_LEN) return false;
    if (s.in_start < 0 || s.in_start > n_in - 1) return false;
    if ((s.out_len - 1) * (int64_t)s.num / s.den > n_in - 1 - s.in_start) return false;           // the last read
    if (s.out_off < 0 || s.out_off > n_out || s.out_len > n_out - s.out_off) return false;
    return true;
}

struct RetimeStage {
    std::vector<RetimeSeg> image;     // the table as uploaded
    int64_t n_tiles;
    unsigned grid;
};

// `out_addr`: the device address of output sample 0 (the chunks lie on the grid of 16-byte-aligned ADDRESSES).  EINVAL: an unknown
// dtype, no segment, an empty input or output, a segment that segment_ok refuses (`out` is then unspecified).
inline int stage_retime(const SushiHipRetimeSegment* seg, int n_seg, int dtype, int64_t n_in, int64_t n_out, uintptr_t out_addr, RetimeStage& out) {
    if (!row_dtype_ok(dtype)) return SUSHI_HIP_EINVAL;
    if (n_seg < 1 || n_in < 1 || n_out < 1) return SUSHI_HIP_EINVAL;
    for (int k = 0; k < n_seg; ++k)
        if (!segment_ok(seg[k], n_in, n_out)) return SUSHI_HIP_EINVAL;
    const int size = row_sample_size(dtype), per = size == 1 ? RetimeChunk<uint8_t>::PER : RetimeChunk<float>::PER;
    out.image.resize((size_t)n_seg);
    int64_t tiles = 0;
    for (int k = 0; k < n_seg; ++k) {
        const SushiHipRetimeSegment& s = seg[k];
        RetimeSeg& d = out.image[k];
        d.in_start = s.in_start; d.out_off = s.out_off; d.out_len = s.out_len; d.num = s.num; d.den = s.den;
        d.phase = (int32_t)(((out_addr + (uint64_t)s.out_off * size) & 15) / size);
        d.reserved = 0;
        d.first_tile = tiles;
        const int64_t chunks = (s.out_len + d.phase + per - 1) / per;
        tiles += (chunks + RETIME_THREADS - 1) / RETIME_THREADS;
    }
    out.n_tiles = tiles;
    out.grid = (unsigned)(tiles < RETIME_MAX_GRID ? tiles : RETIME_MAX_GRID);
    return SUSHI_HIP_OK;
}

}  // namespace sushi
#endif
