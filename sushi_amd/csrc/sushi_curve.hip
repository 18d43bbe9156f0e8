// sushi_amd/csrc/sushi_curve.hip -- whole match-score curves: the row cv2.matchTemplate returns (wav.py:185 `result`), not
// only its arg-min.  Every position of a curve is computed; none can be excluded, so the work is O(P M) and runs on the
// pipe that suits the sample type:
//   * uint8 streams: the centred cross term as an exact integer GEMM with one Toeplitz operand on v_mfma_i32_32x32x32_i8;
//   * float32 streams: the canonical float64 chain of the exact stages (sushi_exact.hip refine_kernel / exact_tiles_kernel)
//     on the VALU.
// Either way each value is bit for bit what the exact stages produce for that position.  The tile bodies
// (curve_tiles.hpp) also evaluate the listed block pairs of a threshold run (sushi_hip_batch_run_threshold):
// threshold_tiles_kernel, launched from sushi_fft.hip through launch_threshold_tiles; and those of a best-K run
// (sushi_hip_batch_run_best): best_tiles_kernel and best_select_kernel.  What those three share is written once,
// in front of them: the decoding of a work item (ListedPairs -> listed_tile), a tile's evaluation with an epilogue (eval_tile),
// the threshold test (passes), the launch by sample type (launch_by_dtype).
//
// Stateless: no handle, no spectra; the request table and the tile queue live in the caller's workspace.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "../../include/sushi_hip.h"
#include "sushi_common.hpp"
#include "sushi_internal.hpp"
#include "curve_tiles.hpp"
#include "curve_core.hpp"

namespace {

using namespace sushi;
using namespace sushi_tiles;

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
// The listed block pairs of a threshold run and of a best-K run: every position of them, exactly, a TILE of a pair per work item
// (item = list slot x TILES_PER_PAIR + tile: the tiles of a pair run side by side and share its pattern in the L2).  The same tile
// bodies as the curves, so a score is the curve's value at that position, bit for bit.  A tile is 1024 positions for both sample
// types (f32_tile<4>).  First what the kernels of both runs share: which tile a work item is, and its evaluation.
// ------------------------------------------------------------------------------------------------------------------------
static_assert(TILE == U8_TILE && TILE == 256 * 4 && TILE / 32 == 32, "a tile's hit bits are 32 words");

__device__ __forceinline__ TileSrc tile_src(const StreamRefs& r, const int method) {
    return TileSrc{r.dst_raw, r.dst_s1, r.dst_s2, r.dst_len, r.src_raw, r.src_s1, r.src_s2, r.centre, method};
}
__device__ __forceinline__ TileReq tile_req(const SearchDesc& sd) { return TileReq{sd.tmpl_off, sd.win_start, sd.tmpl_len, sd.n_pos}; }

// the work items of a list: every tile of every listed pair.  (Every list holds distinct pairs of the sub-batch and list_max is the
// sub-batch's pair count, so the clamp never bites.)
__device__ __forceinline__ int64_t listed_items(const ListedPairs& a) {
    const int n_list = a.list_count ? min(*a.list_count, a.list_max) : a.list_max;
    return (int64_t)n_list * TILES_PER_PAIR;
}

// One work item: tile `t` of the pair `pr` in list slot item / TILES_PER_PAIR, of search `k` (of the sub-batch); p0: the tile's first
// position in request coordinates; row: the pair's; valid (uniform): the tile holds a position of the window
struct ListedTile { int pr, k, t; int64_t p0; TileReq rq; uint32_t* row; bool valid; };
__device__ __forceinline__ ListedTile listed_tile(const ListedPairs& a, const int64_t item) {
    ListedTile x;
    x.t = (int)(item % TILES_PER_PAIR);
    x.pr = a.list[(int)(item / TILES_PER_PAIR)];
    x.k = a.pairmap[x.pr];
    const SearchDesc sd = a.searches[x.k];
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const int64_t pairI = absolute_pair(lay, a.sub_first_pair, x.pr, sd);
    x.p0 = pairI * FFT_STEP * (int64_t)FFT_SEG + (int64_t)x.t * TILE - sd.win_start;
    x.rq = tile_req(sd);
    x.row = a.rows + (size_t)x.pr * THR_SLOT_WORDS;
    x.valid = x.p0 + TILE > 0 && x.p0 < sd.n_pos;
    return x;
}

// A tile evaluated with `emit` (curve_tiles.hpp).  Every thread of the workgroup calls it: the tile bodies hold barriers.  `lds`:
// LISTED_LDS_DOUBLES<U8> doubles, free of readers (the callers' barrier at the top of an item).
template <bool U8> constexpr int LISTED_LDS_DOUBLES = U8 ? 4 * U8_TILE : XG * XM + f32_li_doubles<4>();
template <bool U8, class Emit>
__device__ __forceinline__ void eval_tile(const TileSrc& src, const TileReq& rq, const int64_t p0, double* lds, Emit&& emit) {
    if constexpr (U8) u8_tile(src, rq, p0, reinterpret_cast<double(*)[U8_TILE]>(lds), emit);
    else f32_tile<4>(src, rq, p0, lds, lds + XG * XM, emit);
}

// whether a score passes the caller's threshold: at most it (TM_SQDIFF_NORMED), at least it (TM_CCOEFF_NORMED)
__device__ __forceinline__ bool passes(const float v, const double threshold, const bool cc) {
    return cc ? (double)v >= threshold : (double)v <= threshold;
}

// ------------------------------------------------------------------------------------------------------------------------
// Threshold run:
//   pass 0: the tile's hit bits (THR_MASK), its hit count (THR_COUNT) and its smallest ranking score (THR_MIN: the bound's audit)
//           into the pair's row -- every word of the tile, plain stores, so nothing has to be cleared first;
//   pass 1: tiles with hits, after thr_scan_kernel (sushi_fft_threshold.inc) has left each pair's first output slot (THR_OFF):
//           evaluated again, every hit to its slot -- the pair's slot + the hits of the tiles before + the set bits before it.
// ------------------------------------------------------------------------------------------------------------------------
template <bool U8>
__global__ __launch_bounds__(256)
void threshold_tiles_kernel(ThresholdTileParams a) {
    __shared__ double lds[LISTED_LDS_DOUBLES<U8>];
    __shared__ unsigned mask[TILE / 32];
    __shared__ int wpre[TILE / 32];
    __shared__ unsigned red_min;
    const int tid = threadIdx.x;
    const TileSrc src = tile_src(a.lp.r, a.lp.method);
    const bool cc = a.lp.method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const int64_t n_items = listed_items(a.lp);
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const ListedTile x = listed_tile(a.lp, it);
        const int t = x.t;
        uint32_t* __restrict__ row = x.row;
        __syncthreads();                                                    // the previous item's LDS is consumed
        if (a.pass == 0) {
            if (tid < TILE / 32) mask[tid] = 0u;
            if (tid == 0) red_min = 0x7f800000u;                            // +inf (ranking scores are >= 0: uint order is float order)
            __syncthreads();
            float my_min = __builtin_inff();
            if (x.valid)
                eval_tile<U8>(src, x.rq, x.p0, lds, [&](int i, int64_t, float v) {
                    if (passes(v, a.threshold, cc)) atomicOr(&mask[i >> 5], 1u << (i & 31));
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
            if (cnt == 0 || !x.valid) continue;                             // (uniform)
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
            SushiHipHit* __restrict__ out = a.hits + (size_t)(a.lp.first_search + x.k) * (size_t)a.capacity;
            eval_tile<U8>(src, x.rq, x.p0, lds, [&](int i, int64_t p, float v) {
                const unsigned m = mask[i >> 5];
                if ((m >> (i & 31)) & 1u) {
                    const int off = before + wpre[i >> 5] + __popc(m & ((1u << (i & 31)) - 1u));
                    if (off < a.capacity) out[off] = SushiHipHit{(int32_t)p, v};
                }
            });
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Best-K run: the first K picks of greedy suppression over every search's whole score row, from the listed block
// pairs alone.
//   best_tiles_kernel   per tile of a listed pair: its best eligible position as a pick key (BEST_KEY) and its smallest ranking
//                       score over all positions (THR_MIN) into the pair's row -- plain stores of every word a later kernel reads;
//   best_select_kernel  a workgroup per search, K rounds: the smallest key over the evaluated pairs' tiles is the pick; tiles
//                       wholly inside the pick's window (g - S, g + S) are dead, the at most two tiles the window's edges cut are
//                       evaluated again with every pick so far masked (BEST_WORK is what the rounds read and write; BEST_KEY stays
//                       as evaluated, for the next selection over more pairs).
// ------------------------------------------------------------------------------------------------------------------------
// the smaller key is the better pick: (score under the order-preserving map of float bits, negated for TM_CCOEFF_NORMED) | index
// | whether the score is -0.0 (0.0 and -0.0 are one value to the order, as to NumPy's; the bit gives the curve's bits back)
__device__ __forceinline__ unsigned long long pick_key(const float v, const int64_t p, const bool cc) {
    const unsigned u = ordered_bits(cc ? -(v + 0.0f) : v + 0.0f);
    return ((unsigned long long)u << 32) | ((unsigned long long)p << 1) | (__float_as_uint(v) == 0x80000000u ? 1ull : 0ull);
}
__device__ __forceinline__ int32_t pick_index(const unsigned long long key) { return (int32_t)((key & 0xffffffffull) >> 1); }
__device__ __forceinline__ float pick_score(const unsigned long long key, const bool cc) {
    if (key & 1ull) return -0.0f;
    const float s = ordered_bits_inv((unsigned)(key >> 32));
    return cc ? -s : s;
}
// the ranking score the pair bound is a lower bound of (the score; 1 - the coefficient formed in double), rounded UP to a float
__device__ __forceinline__ float rank_up(const float v, const bool cc) {
    if (!cc) return v;
    const double u = 1.0 - (double)v;
    float f = (float)u;
    if ((double)f < u) f = f >= 0.f ? __uint_as_float(__float_as_uint(f + 0.0f) + 1u) : __uint_as_float(__float_as_uint(f) - 1u);
    return fmaxf(f, 0.f);
}

template <bool U8>
__global__ __launch_bounds__(256)
void best_tiles_kernel(BestParams a) {
    __shared__ double lds[LISTED_LDS_DOUBLES<U8>];
    __shared__ unsigned long long red4[4];
    __shared__ unsigned red_min;
    const int tid = threadIdx.x;
    const TileSrc src = tile_src(a.lp.r, a.lp.method);
    const bool cc = a.lp.method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const int64_t n_items = listed_items(a.lp);
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const ListedTile x = listed_tile(a.lp, it);
        __syncthreads();                                                    // the previous item's LDS is consumed
        if (tid == 0) red_min = 0x7f800000u;                                // +inf (ranking scores are >= 0: uint order is float order)
        unsigned long long my_key = NO_KEY;
        float my_min = __builtin_inff();
        if (x.valid)
            eval_tile<U8>(src, x.rq, x.p0, lds, [&](int, int64_t p, float v) {
                const bool ok = !a.has_threshold || passes(v, a.threshold, cc);
                const unsigned long long key = pick_key(v, p, cc);
                if (ok && key < my_key) my_key = key;
                my_min = fminf(my_min, rank_up(v, cc));
            });
        const unsigned long long best = block_min_u64(my_key, red4);        // (its barriers also order red_min's reset and use)
        atomicMin(&red_min, __float_as_uint(my_min));                       // (LDS: once per thread, after the tile)
        __syncthreads();
        if (tid == 0) {
            reinterpret_cast<unsigned long long*>(x.row + BEST_KEY)[x.t] = best;
            x.row[THR_MIN + x.t] = red_min;
        }
    }
}

template <bool U8>
__global__ __launch_bounds__(256)
void best_select_kernel(BestParams a) {
    __shared__ double lds[LISTED_LDS_DOUBLES<U8>];
    __shared__ unsigned long long red4[4];
    __shared__ int64_t picks[BEST_MAX_K];
    const int tid = threadIdx.x;
    const int k = blockIdx.x;
    if (k == 0 && tid == 0) {
        if (a.reset0) *a.reset0 = 0;
        if (a.reset1) *a.reset1 = 0;
    }
    const int gk = a.lp.first_search + k;                                   // the search's global index
    if (a.stamp_flags && a.stamp_flags[gk] != a.stamp) return;              // (uniform) nothing new for this search
    const TileSrc src = tile_src(a.lp.r, a.lp.method);
    const bool cc = a.lp.method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const SearchDesc sd = a.lp.searches[k];
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const TileReq rq = tile_req(sd);
    const int pr0 = sd.first_pair - a.lp.sub_first_pair;
    const int64_t S = a.min_separation > 0 ? a.min_separation : sd.tmpl_len;
    const int K = a.k;
    SushiHipHit* __restrict__ out = a.hits + (size_t)gk * (size_t)K;
    auto evaluated = [&](const int i) { return !a.audit_mark || (a.audit_mark[pr0 + i] & MARK_LISTED) != 0; };
    auto keys_of = [&](const int i, const int what) {
        return reinterpret_cast<unsigned long long*>(a.lp.rows + (size_t)(pr0 + i) * THR_SLOT_WORDS + what);
    };
    // what the rounds work on: every evaluated tile as it was evaluated
    for (int i = tid; i < lay.n_pairs; i += 256)
        if (evaluated(i)) {
            const unsigned long long* __restrict__ o = keys_of(i, BEST_KEY);
            unsigned long long* __restrict__ w = keys_of(i, BEST_WORK);
            for (int t = 0; t < TILES_PER_PAIR; ++t) w[t] = o[t];
        }
    __syncthreads();
    int n_picks = 0;
    float last = 0.f;
    for (int j = 0; j < K; ++j) {
        unsigned long long mine = NO_KEY;
        for (int i = tid; i < lay.n_pairs; i += 256)
            if (evaluated(i)) {
                const unsigned long long* __restrict__ w = keys_of(i, BEST_WORK);
                for (int t = 0; t < TILES_PER_PAIR; ++t) mine = w[t] < mine ? w[t] : mine;
            }
        const unsigned long long best = block_min_u64(mine, red4);
        if (best == NO_KEY) break;                                          // (uniform) nothing eligible is left
        const int64_t g = pick_index(best);
        last = pick_score(best, cc);
        if (tid == 0) { picks[j] = g; out[j] = SushiHipHit{(int32_t)g, last}; }
        n_picks = j + 1;
        if (n_picks == K) break;
        __syncthreads();                                                    // picks[j] is there
        // the pick's window (g - S, g + S), cut to the row: tiles wholly inside are dead, the tiles that hold its ends are looked at
        const int64_t lo = max((int64_t)0, g - S + 1), hi = min((int64_t)sd.n_pos - 1, g + S - 1);
        const int64_t a_lo = (lo + sd.win_start) / TILE, a_hi = (hi + sd.win_start) / TILE;       // (tiles of the absolute grid)
        auto tile_keys = [&](const int64_t at, int* t) -> unsigned long long* {
            const int64_t i = at / TILES_PER_PAIR - lay.pair0;
            *t = (int)(at % TILES_PER_PAIR);
            return i >= 0 && i < lay.n_pairs && evaluated((int)i) ? keys_of((int)i, BEST_WORK) : nullptr;
        };
        for (int64_t at = a_lo + 1 + tid; at < a_hi; at += 256) {
            int t;
            unsigned long long* w = tile_keys(at, &t);
            if (w) w[t] = NO_KEY;
        }
        for (int e = 0; e < (a_hi > a_lo ? 2 : 1); ++e) {
            const int64_t at = e ? a_hi : a_lo;
            int t;
            unsigned long long* w = tile_keys(at, &t);                      // (uniform)
            if (!w) continue;
            const int64_t p0 = at * TILE - sd.win_start;
            const int64_t t_lo = max((int64_t)0, p0), t_hi = min((int64_t)sd.n_pos - 1, p0 + TILE - 1);
            // (through the reduction: one value for every thread whatever each of them read, and its barriers order the earlier
            // stores to w[t] and the tile body's use of the LDS)
            if (block_min_u64(w[t], red4) == NO_KEY) continue;              // dead already, or nothing eligible in it
            if (t_lo >= lo && t_hi <= hi) {
                __syncthreads();
                if (tid == 0) w[t] = NO_KEY;
                continue;
            }
            unsigned long long my_key = NO_KEY;
            eval_tile<U8>(src, rq, p0, lds, [&](int, int64_t p, float v) {
                bool ok = !a.has_threshold || passes(v, a.threshold, cc);
                for (int q = 0; q <= j; ++q) {
                    const int64_t d = p - picks[q];
                    ok = ok && (d >= S || -d >= S);
                }
                const unsigned long long key = pick_key(v, p, cc);
                if (ok && key < my_key) my_key = key;
            });
            const unsigned long long tb = block_min_u64(my_key, red4);
            if (tid == 0) w[t] = tb;
        }
        __syncthreads();                                                    // the round's stores are there for the next one's loads
    }
    if (tid == 0) {
        a.counts[gk] = n_picks;
        // what a pair's bound has to stay above from now on: the K-th pick's ranking score, or the threshold's where that is tighter
        unsigned long long key = a.tkey;
        if (n_picks == K) {
            const float u = rank_up(last, cc);
            if (a.tkey == NO_KEY || u < key_score(a.tkey)) key = ((unsigned long long)__float_as_uint(u) << 32) | 0xffffffffull;
        }
        a.gkeys[gk] = key;
    }
}

// a kernel of 256 threads in its uint8 or its float32 form, by the streams' sample type
template <class Params>
int launch_by_dtype(const int dtype, void (*u8)(Params), void (*f32)(Params), const unsigned grid, const Params& p, hipStream_t st) {
    hipLaunchKernelGGL(dtype == SUSHI_HIP_U8 ? u8 : f32, dim3(grid), dim3(256), 0, st, p);
    return launch_ok();
}

// a fixed grid striding over a list's items (their number is on the device): 256 CUs, a few workgroups each
unsigned listed_grid(const ListedPairs& lp) {
    return (unsigned)std::min<int64_t>((int64_t)std::max(lp.list_max, 1) * TILES_PER_PAIR, 2048);
}

}  // namespace

namespace sushi {

int launch_threshold_tiles(const ThresholdTileParams& p, hipStream_t st) {
    return launch_by_dtype(p.lp.r.dtype, threshold_tiles_kernel<true>, threshold_tiles_kernel<false>, listed_grid(p.lp), p, st);
}

int launch_best_tiles(const BestParams& p, hipStream_t st) {
    return launch_by_dtype(p.lp.r.dtype, best_tiles_kernel<true>, best_tiles_kernel<false>, listed_grid(p.lp), p, st);
}

int launch_best_select(const BestParams& p, hipStream_t st) {
    return launch_by_dtype(p.lp.r.dtype, best_select_kernel<true>, best_select_kernel<false>, (unsigned)p.n_sub, p, st);
}

}  // namespace sushi

extern "C" {

size_t sushi_hip_curve_bytes(const SushiHipRequest* req_host, int n) {
    (void)req_host;                   // (the workspace depends on the number of requests only)
    return curve_layout_bytes(n);
}

int sushi_hip_match_curves(const SushiHipStream* dst, const SushiHipStream* src, const SushiHipRequest* req_host, int n,
                           int method, void* mem_dev, size_t mem_bytes, float* out_dev, void* hip_stream) { return c_boundary([&]() -> int {
    if (!dst || !src || !req_host || !mem_dev || !out_dev || n < 0) return SUSHI_HIP_EINVAL;
    if (!method_known(method)) return SUSHI_HIP_EINVAL;
    if (n == 0) return SUSHI_HIP_OK;
    if (dst->dtype != src->dtype) return SUSHI_HIP_EINVAL;           // cv2.matchTemplate asserts equal types
    CurveStage staged;
    const int rc = stage_curves(req_host, n, dst->dtype, dst->n, src->n, staged);
    if (rc != SUSHI_HIP_OK) return rc;
    if (((uintptr_t)mem_dev & 255) || ((uintptr_t)out_dev & 3)) return SUSHI_HIP_EALIGN;
    if (mem_bytes < staged.image.size()) return SUSHI_HIP_ENOSPACE;

    hipStream_t st = (hipStream_t)hip_stream;
    char* mem = (char*)mem_dev;
    // (The source is pageable host memory that dies with this call.  ASSUMED: the runtime has taken its copy of such a source when
    // hipMemcpyAsync returns.)
    if (hipMemcpyAsync(mem, staged.image.data(), staged.image.size(), hipMemcpyHostToDevice, st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    CurveArgs a;
    a.src = TileSrc{dst->raw, dst->s1, dst->s2, dst->n, src->raw, src->s1, src->s2, sushi_hip_centre(dst->dtype), method};
    a.desc = reinterpret_cast<const CurveDesc*>(mem + CURVE_HEAD);
    a.n = n; a.n_items = staged.n_items;
    a.queue = reinterpret_cast<unsigned long long*>(mem);
    a.out = out_dev;
    if (dst->dtype == SUSHI_HIP_U8) hipLaunchKernelGGL(curve_u8_kernel, dim3(staged.grid), dim3(256), 0, st, a);
    else if (staged.per_item == CURVE_F32_ITEM) hipLaunchKernelGGL(curve_f32_kernel<CURVE_F32_ITEM / 256>, dim3(staged.grid), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(curve_f32_kernel<CURVE_F32_SMALL_ITEM / 256>, dim3(staged.grid), dim3(256), 0, st, a);
    return launch_ok();
}); }

}  // extern "C"
