// sushi_amd/csrc/sushi_retime.hip -- sushi_hip_retime: a stream read at another speed (gfx950).
//
// Linear interpolation at a rational step num / den per output sample, in the arithmetic include/sushi_hip.h states and
// retime_core.hpp implements (float64, product and sum rounded separately: this unit is compiled with -ffp-contract=off), so
// that the output is bit-identical to the NumPy restatement (sushi_amd/retime.py retime_host).
//
// One launch serves a table of segments: many short ones (the probes of estimate_speed) or one of a whole stream.  A segment's
// outputs are cut into chunks of PER consecutive samples, one per thread, on the grid of 16-byte-aligned output ADDRESSES (the
// chunk that holds a segment's first output starts up to 15 bytes in front of it), 256 chunks to a tile; a workgroup finds its
// tile's segment by bisection of the tiles' running count.  A thread divides once (retime_seek) and advances incrementally.
// Whole chunks leave as 16-byte stores; reads are two neighbouring samples per output, a wave's within a few cache lines.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>
#include <vector>

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "retime_core.hpp"

namespace {

using sushi::align_up;
using sushi::launch_ok;

// a segment on the device
struct RetimeSeg {
    int64_t in_start, out_off, out_len;
    int64_t first_tile;       // tiles of the segments before this one
    int32_t num, den;
    int32_t phase;            // samples between the 16-byte boundary at or in front of the segment's first output and that output
    int32_t reserved;
};
static_assert(sizeof(RetimeSeg) == 48, "RetimeSeg layout");

struct RetimeArgs {
    const void* in;
    int64_t n_in;
    const RetimeSeg* seg;
    int n_seg;
    int64_t n_tiles;
    void* out;
};

template <class T> struct RetimeChunk;
template <> struct RetimeChunk<float> { static constexpr int PER = 8; };        // two 16-byte stores
template <> struct RetimeChunk<uint8_t> { static constexpr int PER = 16; };     // one
constexpr int RETIME_THREADS = 256;

inline size_t retime_layout_bytes(int n_seg) { return n_seg < 1 ? 0 : align_up((size_t)n_seg * sizeof(RetimeSeg), 256); }

template <class T>
__global__ __launch_bounds__(RETIME_THREADS)
void retime_kernel(RetimeArgs a) {
    constexpr int PER = RetimeChunk<T>::PER;
    const T* __restrict__ x = (const T*)a.in;
    T* __restrict__ out = (T*)a.out;
    for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        int lo = 0, hi = a.n_seg - 1;                       // the last segment whose first tile is not behind `tile`
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.seg[mid].first_tile <= tile) lo = mid; else hi = mid - 1;
        }
        const RetimeSeg sg = a.seg[lo];
        const int64_t chunk = (tile - sg.first_tile) * RETIME_THREADS + threadIdx.x;
        const int64_t c0 = chunk * PER - sg.phase;          // first output of the chunk (the segment's first chunk starts in front of output 0)
        const int64_t i0 = c0 > 0 ? c0 : 0;
        const int64_t i1 = c0 + PER < sg.out_len ? c0 + PER : sg.out_len;
        if (i0 >= i1) continue;
        sushi::RetimeCursor c = sushi::retime_seek(sg.in_start, i0, sg.num, sg.den);
        const int32_t qstep = sg.num / sg.den, rstep = sg.num % sg.den;
        T* __restrict__ o = out + sg.out_off + i0;
        if (i1 - i0 == PER) {
            struct alignas(16) Pack { T v[PER]; } pk;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                pk.v[k] = sushi::retime_sample<T>(x, a.n_in, c.j, c.r, sg.den);
                sushi::retime_advance(c, qstep, rstep, sg.den);
            }
            const uint4* __restrict__ pv = reinterpret_cast<const uint4*>(&pk);
            uint4* __restrict__ po = reinterpret_cast<uint4*>(o);           // 16-byte aligned: c0 lies on the address grid
#pragma unroll
            for (int k = 0; k < (int)(sizeof(Pack) / 16); ++k) po[k] = pv[k];
        } else {
            for (int64_t i = i0; i < i1; ++i) {
                o[i - i0] = sushi::retime_sample<T>(x, a.n_in, c.j, c.r, sg.den);
                sushi::retime_advance(c, qstep, rstep, sg.den);
            }
        }
    }
}

constexpr int32_t RETIME_MAX_TERM = 1 << 20;             // num, den
constexpr int64_t RETIME_MAX_LEN = (int64_t)1 << 40;     // out_len (i * num stays below 2^60)

bool segment_ok(const SushiHipRetimeSegment& s, int64_t n_in, int64_t n_out) {
    if (s.num < 1 || s.num > RETIME_MAX_TERM || s.den < 1 || s.den > RETIME_MAX_TERM) return false;
    if ((int64_t)s.num > 8 * (int64_t)s.den || (int64_t)s.den > 8 * (int64_t)s.num) return false;
    if (s.out_len < 1 || s.out_len >= RETIME_MAX_LEN) return false;
    if (s.in_start < 0 || s.in_start > n_in - 1) return false;
    if ((s.out_len - 1) * (int64_t)s.num / s.den > n_in - 1 - s.in_start) return false;           // the last read
    if (s.out_off < 0 || s.out_off > n_out || s.out_len > n_out - s.out_off) return false;
    return true;
}

}  // namespace

extern "C" {

size_t sushi_hip_retime_bytes(int n_seg) { return retime_layout_bytes(n_seg); }

int sushi_hip_retime(const void* in_dev, int dtype, int64_t n_in, const SushiHipRetimeSegment* seg_host, int n_seg,
                     void* out_dev, int64_t n_out, void* mem_dev, size_t mem_bytes, void* hip_stream) try {
    if (!in_dev || !seg_host || !out_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    if (dtype != SUSHI_HIP_U8 && dtype != SUSHI_HIP_F32) return SUSHI_HIP_EINVAL;
    if (n_seg < 1 || n_in < 1 || n_out < 1) return SUSHI_HIP_EINVAL;
    for (int k = 0; k < n_seg; ++k)
        if (!segment_ok(seg_host[k], n_in, n_out)) return SUSHI_HIP_EINVAL;
    const bool u8 = dtype == SUSHI_HIP_U8;
    const int size = u8 ? 1 : 4, per = u8 ? RetimeChunk<uint8_t>::PER : RetimeChunk<float>::PER;
    if (((uintptr_t)mem_dev & 255) || ((uintptr_t)in_dev & (size - 1)) || ((uintptr_t)out_dev & (size - 1))) return SUSHI_HIP_EALIGN;
    if (mem_bytes < retime_layout_bytes(n_seg)) return SUSHI_HIP_ENOSPACE;

    std::vector<RetimeSeg> up((size_t)n_seg);
    int64_t tiles = 0;
    for (int k = 0; k < n_seg; ++k) {
        const SushiHipRetimeSegment& s = seg_host[k];
        RetimeSeg& d = up[k];
        d.in_start = s.in_start; d.out_off = s.out_off; d.out_len = s.out_len; d.num = s.num; d.den = s.den;
        d.phase = (int32_t)((((uintptr_t)out_dev + (uint64_t)s.out_off * size) & 15) / size);
        d.reserved = 0;
        d.first_tile = tiles;
        const int64_t chunks = (s.out_len + d.phase + per - 1) / per;
        tiles += (chunks + RETIME_THREADS - 1) / RETIME_THREADS;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    // (a pageable source: the runtime has staged it when the call returns, as for sushi_hip_match_curves' descriptors)
    if (hipMemcpyAsync(mem_dev, up.data(), up.size() * sizeof(RetimeSeg), hipMemcpyHostToDevice, st) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    RetimeArgs a;
    a.in = in_dev; a.n_in = n_in; a.seg = (const RetimeSeg*)mem_dev; a.n_seg = n_seg; a.n_tiles = tiles; a.out = out_dev;
    // a fixed grid striding over the tiles: 256 CUs, eight workgroups each (a CU holds eight of these)
    const unsigned grid = (unsigned)(tiles < 2048 ? tiles : 2048);
    if (u8) hipLaunchKernelGGL(retime_kernel<uint8_t>, dim3(grid), dim3(RETIME_THREADS), 0, st, a);
    else hipLaunchKernelGGL(retime_kernel<float>, dim3(grid), dim3(RETIME_THREADS), 0, st, a);
    return launch_ok();
} catch (const std::bad_alloc&) { return SUSHI_HIP_ENOMEM; } catch (...) { return SUSHI_HIP_EINTERNAL; }

}  // extern "C"
