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

#include "../../include/sushi_hip.h"
#include "sushi_internal.hpp"
#include "retime_core.hpp"

namespace {

using namespace sushi;

struct RetimeArgs {
    const void* in;
    int64_t n_in;
    const RetimeSeg* seg;
    int n_seg;
    int64_t n_tiles;
    void* out;
};

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
        RetimeCursor c = retime_seek(sg.in_start, i0, sg.num, sg.den);
        const int32_t qstep = sg.num / sg.den, rstep = sg.num % sg.den;
        T* __restrict__ o = out + sg.out_off + i0;
        if (i1 - i0 == PER) {
            struct alignas(16) Pack { T v[PER]; } pk;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                pk.v[k] = retime_sample<T>(x, a.n_in, c.j, c.r, sg.den);
                retime_advance(c, qstep, rstep, sg.den);
            }
            const uint4* __restrict__ pv = reinterpret_cast<const uint4*>(&pk);
            uint4* __restrict__ po = reinterpret_cast<uint4*>(o);           // 16-byte aligned: c0 lies on the address grid
#pragma unroll
            for (int k = 0; k < (int)(sizeof(Pack) / 16); ++k) po[k] = pv[k];
        } else {
            for (int64_t i = i0; i < i1; ++i) {
                o[i - i0] = retime_sample<T>(x, a.n_in, c.j, c.r, sg.den);
                retime_advance(c, qstep, rstep, sg.den);
            }
        }
    }
}

}  // namespace

extern "C" {

size_t sushi_hip_retime_bytes(int n_seg) { return retime_layout_bytes(n_seg); }

int sushi_hip_retime(const void* in_dev, int dtype, int64_t n_in, const SushiHipRetimeSegment* seg_host, int n_seg,
                     void* out_dev, int64_t n_out, void* mem_dev, size_t mem_bytes, void* hip_stream) { return c_boundary([&]() -> int {
    if (!in_dev || !seg_host || !out_dev || !mem_dev) return SUSHI_HIP_EINVAL;
    RetimeStage staged;
    const int rc = stage_retime(seg_host, n_seg, dtype, n_in, n_out, (uintptr_t)out_dev, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if (((uintptr_t)mem_dev & 255) || !row_aligned(in_dev, dtype) || !row_aligned(out_dev, dtype)) return SUSHI_HIP_EALIGN;
    if (mem_bytes < retime_layout_bytes(n_seg)) return SUSHI_HIP_ENOSPACE;

    hipStream_t st = (hipStream_t)hip_stream;
    // (The source is pageable host memory that dies with this call.  ASSUMED: the runtime has taken its copy of such a source when
    // hipMemcpyAsync returns.)
    if (hipMemcpyAsync(mem_dev, staged.image.data(), staged.image.size() * sizeof(RetimeSeg), hipMemcpyHostToDevice, st) != hipSuccess)
        return SUSHI_HIP_ELAUNCH;
    RetimeArgs a;
    a.in = in_dev; a.n_in = n_in; a.seg = (const RetimeSeg*)mem_dev; a.n_seg = n_seg; a.n_tiles = staged.n_tiles; a.out = out_dev;
    row_dispatch(dtype, [&](auto t) { hipLaunchKernelGGL(retime_kernel<decltype(t)>, dim3(staged.grid), dim3(RETIME_THREADS), 0, st, a); });
    return launch_ok();
}); }

}  // extern "C"
