// sushi_amd/csrc/sushi_curve.hip -- whole match-score curves: the row cv2.matchTemplate returns (wav.py:185 `result`), not
// only its arg-min.  Every position of a curve is computed; none can be excluded, so the work is O(P M) and runs on the
// pipe that suits the sample type:
//   * uint8 streams: the centred cross term as an exact integer GEMM with one Toeplitz operand on v_mfma_i32_32x32x32_i8;
//   * float32 streams: the canonical float64 chain of the exact stages (sushi_hip.hip refine_kernel / exact_tiles_kernel)
//     on the VALU.
// Either way each value is bit for bit what the exact stages produce for that position.  The tile bodies
// (curve_tiles.hpp) also evaluate the listed block pairs of a threshold run (sushi_hip_batch_run_threshold):
// threshold_tiles_kernel, launched from sushi_fft.hip through launch_threshold_tiles.
//
// Stateless: no handle, no spectra; the request table and the tile queue live in the caller's workspace.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/sushi_hip.h"
#include "sushi_common.hpp"
#include "sushi_internal.hpp"
#include "curve_tiles.hpp"

namespace {

using namespace sushi;
using namespace sushi_tiles;

// One request on the device: where its pattern and window are, where its curve goes, its first work item.
struct CurveDesc {
    int64_t tmpl_off;
    int64_t win_start;
    int64_t out_off;        // first float of its curve in out_dev: sum of n_pos of the requests before it
    int64_t first_item;     // work items of the requests before it
    int32_t tmpl_len;
    int32_t n_pos;
};
static_assert(sizeof(CurveDesc) == 40, "CurveDesc layout");

// workspace: [queue head (u64) | padding to 256 B][CurveDesc x n], uploaded in one copy
constexpr size_t CURVE_HEAD = 256;
size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
size_t curve_layout_bytes(int n) { return n <= 0 ? 0 : CURVE_HEAD + align256((size_t)n * sizeof(CurveDesc)); }

struct CurveArgs {
    TileSrc src;                      // streams, method
    const CurveDesc* desc;
    int n;
    int64_t n_items;
    unsigned long long* queue;
    float* out;
};

// the request holding work item `item`: the last one whose first_item <= item
__device__ __forceinline__ int find_request(const CurveDesc* __restrict__ d, int n, int64_t item) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (d[mid].first_item <= item) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// uint8: one tile of U8_TILE positions per work item (curve_tiles.hpp u8_tile)
__global__ __launch_bounds__(256)
void curve_u8_kernel(CurveArgs a) {
    __shared__ double part[4][U8_TILE];
    __shared__ unsigned long long next_item;
    const int tid = threadIdx.x;
    for (;;) {
        __syncthreads();                                           // the previous item's LDS is consumed
        if (tid == 0) next_item = atomicAdd(a.queue, 1ull);
        __syncthreads();
        const int64_t item = (int64_t)next_item;
        if (item >= a.n_items) break;
        const int k = find_request(a.desc, a.n, item);
        const CurveDesc d = a.desc[k];
        const int64_t p0 = (item - d.first_item) * U8_TILE;
        float* __restrict__ out = a.out + d.out_off;
        u8_tile(a.src, TileReq{d.tmpl_off, d.win_start, d.tmpl_len, d.n_pos}, p0, part,
                [&](int, int64_t p, float v) { out[p] = v; });
    }
}

// float32: 256 NPOS positions per work item (curve_tiles.hpp f32_tile)
template <int NPOS>
__global__ __launch_bounds__(256)
void curve_f32_kernel(CurveArgs a) {
    __shared__ double lt[XG * XM];
    __shared__ double li[f32_li_doubles<NPOS>()];
    __shared__ unsigned long long next_item;
    const int tid = threadIdx.x;
    for (;;) {
        __syncthreads();
        if (tid == 0) next_item = atomicAdd(a.queue, 1ull);
        __syncthreads();
        const int64_t item = (int64_t)next_item;
        if (item >= a.n_items) break;
        const int k = find_request(a.desc, a.n, item);
        const CurveDesc d = a.desc[k];
        const int64_t p0 = (item - d.first_item) * (256 * NPOS);
        float* __restrict__ out = a.out + d.out_off;
        f32_tile<NPOS>(a.src, TileReq{d.tmpl_off, d.win_start, d.tmpl_len, d.n_pos}, p0, lt, li,
                       [&](int, int64_t p, float v) { out[p] = v; });
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Threshold run: every position of the listed block pairs, exactly, a TILE of a pair per work item (item =
// list slot x TILES_PER_PAIR + tile: the tiles of a pair run side by side and share its pattern in the L2).  The same tile bodies
// as the curves, so a hit's score is the curve's value at that position, bit for bit.
//   pass 0: the tile's hit bits (THR_MASK), its hit count (THR_COUNT) and its smallest ranking score (THR_MIN: the bound's audit)
//           into the pair's row -- every word of the tile, plain stores, so nothing has to be cleared first;
//   pass 1: tiles with hits, after thr_scan_kernel (sushi_fft_threshold.inc) has left each pair's first output slot (THR_OFF):
//           evaluated again, every hit to its slot -- the pair's slot + the hits of the tiles before + the set bits before it.
// A tile is 1024 positions for both sample types (f32_tile<4>).
// ------------------------------------------------------------------------------------------------------------------------
static_assert(TILE == U8_TILE && TILE == 256 * 4 && TILE / 32 == 32, "a tile's hit bits are 32 words");

template <bool U8>
__global__ __launch_bounds__(256)
void threshold_tiles_kernel(ThresholdTileParams a) {
    constexpr int LDS_DOUBLES = U8 ? 4 * U8_TILE : XG * XM + f32_li_doubles<4>();
    __shared__ double lds[LDS_DOUBLES];
    __shared__ unsigned mask[TILE / 32];
    __shared__ int wpre[TILE / 32];
    __shared__ unsigned red_min;
    const int tid = threadIdx.x;
    const TileSrc src{a.r.dst_raw, a.r.dst_s1, a.r.dst_s2, a.r.dst_len, a.r.src_raw, a.r.src_s1, a.r.src_s2, a.r.centre, a.method};
    const bool cc = a.method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const int n_list = a.list_count ? *a.list_count : a.list_max;
    const int64_t n_items = (int64_t)n_list * TILES_PER_PAIR;
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int slot = (int)(it / TILES_PER_PAIR), t = (int)(it % TILES_PER_PAIR);
        const int pr = a.list[slot];
        const int k = a.pairmap[pr];
        const SearchDesc sd = a.searches[k];
        const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
        const int64_t pairI = lay.pair0 + (a.sub_first_pair + pr - sd.first_pair);
        const int64_t p0 = pairI * FFT_STEP * (int64_t)FFT_SEG + (int64_t)t * TILE - sd.win_start;   // (request coordinates)
        const TileReq rq{sd.tmpl_off, sd.win_start, sd.tmpl_len, sd.n_pos};
        uint32_t* __restrict__ row = a.rows + (size_t)pr * THR_SLOT_WORDS;
        const bool valid = p0 + TILE > 0 && p0 < sd.n_pos;                 // (uniform) the tile holds a position of the window
        auto eval = [&](auto&& emit) {
            if constexpr (U8) u8_tile(src, rq, p0, reinterpret_cast<double(*)[U8_TILE]>(lds), emit);
            else f32_tile<4>(src, rq, p0, lds, lds + XG * XM, emit);
        };
        __syncthreads();                                                    // the previous item's LDS is consumed
        if (a.pass == 0) {
            if (tid < TILE / 32) mask[tid] = 0u;
            if (tid == 0) red_min = 0x7f800000u;                            // +inf (ranking scores are >= 0: uint order is float order)
            __syncthreads();
            float my_min = __builtin_inff();
            if (valid)
                eval([&](int i, int64_t, float v) {
                    const bool hit = cc ? (double)v >= a.threshold : (double)v <= a.threshold;
                    if (hit) atomicOr(&mask[i >> 5], 1u << (i & 31));
                    my_min = fminf(my_min, cc ? 1.0f - v : v);
                });
            atomicMin(&red_min, __float_as_uint(my_min));                 // (LDS: once per thread, after the tile)
            __syncthreads();
            if (tid < 64) {
                const unsigned m = tid < TILE / 32 ? mask[tid] : 0u;
                if (tid < TILE / 32) row[THR_MASK + t * (TILE / 32) + tid] = m;
                int c = __popc(m);
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
                if (tid == 0) { row[THR_COUNT + t] = (uint32_t)c; row[THR_MIN + t] = red_min; }
            }
        } else {
            const int cnt = (int)row[THR_COUNT + t];
            if (cnt == 0 || !valid) continue;                               // (uniform)
            int before = (int)row[THR_OFF];
            for (int u = 0; u < t; ++u) before += (int)row[THR_COUNT + u];
            if (before >= a.capacity) continue;                             // (uniform) nothing of this tile fits
            if (tid < TILE / 32) mask[tid] = row[THR_MASK + t * (TILE / 32) + tid];
            __syncthreads();
            if (tid == 0) {
                int s = 0;
                for (int w = 0; w < TILE / 32; ++w) { wpre[w] = s; s += __popc(mask[w]); }
            }
            __syncthreads();
            SushiHipHit* __restrict__ out = a.hits + (size_t)(a.first_search + k) * (size_t)a.capacity;
            eval([&](int i, int64_t p, float v) {
                const unsigned m = mask[i >> 5];
                if ((m >> (i & 31)) & 1u) {
                    const int off = before + wpre[i >> 5] + __popc(m & ((1u << (i & 31)) - 1u));
                    if (off < a.capacity) out[off] = SushiHipHit{(int32_t)p, v};
                }
            });
        }
    }
}

int launch_ok() { return hipGetLastError() == hipSuccess ? SUSHI_HIP_OK : SUSHI_HIP_ELAUNCH; }

bool request_ok(const SushiHipRequest& r, const SushiHipStream* dst, const SushiHipStream* src) {
    if (r.tmpl_len < 1 || r.n_pos < 1 || r.win_start < 0 || r.tmpl_off < 0) return false;
    if (r.n_pos > 0x7fffffff - 65536 || r.tmpl_len > 0x7fffffff - 65536) return false;
    return r.tmpl_off + r.tmpl_len <= src->n && r.win_start + (int64_t)r.n_pos + r.tmpl_len - 1 <= dst->n;
}

}  // namespace

namespace sushi {

int launch_threshold_tiles(const ThresholdTileParams& p, hipStream_t st) {
    // a fixed grid striding over the items (their number is on the device): 256 CUs, a few workgroups each
    const int64_t want = (int64_t)std::max(p.list_max, 1) * TILES_PER_PAIR;
    const unsigned grid = (unsigned)std::min<int64_t>(want, 2048);
    if (p.r.dtype == SUSHI_HIP_U8) hipLaunchKernelGGL(threshold_tiles_kernel<true>, dim3(grid), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(threshold_tiles_kernel<false>, dim3(grid), dim3(256), 0, st, p);
    return launch_ok();
}

}  // namespace sushi

extern "C" {

size_t sushi_hip_curve_bytes(const SushiHipRequest* req_host, int n) {
    (void)req_host;                   // (the workspace depends on the number of requests only)
    return curve_layout_bytes(n);
}

int sushi_hip_match_curves(const SushiHipStream* dst, const SushiHipStream* src, const SushiHipRequest* req_host, int n,
                           int method, void* mem_dev, size_t mem_bytes, float* out_dev, void* hip_stream) try {
    if (!dst || !src || !req_host || !mem_dev || !out_dev || n < 0) return SUSHI_HIP_EINVAL;
    if (method != SUSHI_HIP_METHOD_SQDIFF_NORMED && method != SUSHI_HIP_METHOD_CCOEFF_NORMED) return SUSHI_HIP_EINVAL;
    if (n == 0) return SUSHI_HIP_OK;
    if (dst->dtype != src->dtype) return SUSHI_HIP_EINVAL;           // cv2.matchTemplate asserts equal types
    for (int k = 0; k < n; ++k)
        if (!request_ok(req_host[k], dst, src)) return SUSHI_HIP_EINVAL;
    if (((uintptr_t)mem_dev & 255) || ((uintptr_t)out_dev & 3)) return SUSHI_HIP_EALIGN;
    if (mem_bytes < curve_layout_bytes(n)) return SUSHI_HIP_ENOSPACE;

    const bool u8 = dst->dtype == SUSHI_HIP_U8;
    // float32: 1024 positions per item where there are enough of them to fill the GPU, else 256 (a quarter of the chains' length
    // each, four times the items)
    int64_t items1024 = 0;
    for (int k = 0; k < n; ++k) items1024 += (req_host[k].n_pos + 1023) / 1024;
    const int per_item = u8 ? U8_TILE : (items1024 >= 2048 ? 1024 : 256);
    std::vector<char> up(curve_layout_bytes(n), 0);                  // queue head 0, then the descriptors
    CurveDesc* d = reinterpret_cast<CurveDesc*>(up.data() + CURVE_HEAD);
    int64_t out_off = 0, items = 0;
    for (int k = 0; k < n; ++k) {
        const SushiHipRequest& r = req_host[k];
        d[k].tmpl_off = r.tmpl_off; d[k].win_start = r.win_start; d[k].tmpl_len = r.tmpl_len; d[k].n_pos = r.n_pos;
        d[k].out_off = out_off; d[k].first_item = items;
        out_off += r.n_pos;
        items += (r.n_pos + per_item - 1) / per_item;
    }
    hipStream_t st = (hipStream_t)hip_stream;
    char* mem = (char*)mem_dev;
    // (a pageable source: the runtime has staged it when the call returns, as for plan_and_upload's descriptors)
    if (hipMemcpyAsync(mem, up.data(), up.size(), hipMemcpyHostToDevice, st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    CurveArgs a;
    a.src = TileSrc{dst->raw, dst->s1, dst->s2, dst->n, src->raw, src->s1, src->s2, sushi_hip_centre(dst->dtype), method};
    a.desc = reinterpret_cast<const CurveDesc*>(mem + CURVE_HEAD);
    a.n = n; a.n_items = items;
    a.queue = reinterpret_cast<unsigned long long*>(mem);
    a.out = out_dev;
    // a fixed grid that takes the items off the queue: 256 CUs, a few workgroups each
    const unsigned grid = (unsigned)(items < 2048 ? items : 2048);
    if (u8) hipLaunchKernelGGL(curve_u8_kernel, dim3(grid), dim3(256), 0, st, a);
    else if (per_item == 1024) hipLaunchKernelGGL(curve_f32_kernel<4>, dim3(grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(curve_f32_kernel<1>, dim3(grid), dim3(256), 0, st, a);
    return launch_ok();
} catch (const std::bad_alloc&) { return SUSHI_HIP_ENOMEM; } catch (...) { return SUSHI_HIP_EINTERNAL; }

}  // extern "C"
