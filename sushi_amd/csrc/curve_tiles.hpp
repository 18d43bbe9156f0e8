// sushi_amd/csrc/curve_tiles.hpp -- the exact tile bodies of the whole-curve kernels (sushi_curve.hip), shared by the curves and by
// the evaluation of listed block pairs in a threshold run and in a best-K run (§3.11; both through sushi_curve.hip's
// eval_tile).  A body evaluates every valid position p in [0, P) of one tile of consecutive positions exactly and hands each value
// to an epilogue, emit(i, p, value), i = p - p0 inside the tile: the curves store it, the threshold run compares it, the best-K
// run keeps the best.  Same arithmetic in the same order every way, so the values are the same bits.
//
// Included by sushi_curve.hip only, which is compiled with -ffp-contract=off (build.py): the epilogue restates cv2's operation
// order, and a fused multiply-add would round differently.
#ifndef SUSHI_CURVE_TILES_HPP
#define SUSHI_CURVE_TILES_HPP

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/sushi_hip.h"
#include "sushi_common.hpp"

namespace sushi_tiles {

using namespace sushi;

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

// What every tile reads: the two streams' samples and float64 prefix sums, the method.
struct TileSrc {
    const void* dst_raw; const double* dst_s1; const double* dst_s2; int64_t dst_len;
    const void* src_raw; const double* src_s1; const double* src_s2;
    double centre;
    int method;
};

// One request: pattern = src[tmpl_off, tmpl_off + M), positions p in [0, P) of the window that starts at win_start.
struct TileReq { int64_t tmpl_off, win_start; int M, P; };

__device__ __forceinline__ float curve_value(const TileSrc& a, const TemplStats& ts, double corr_c_or_u, bool centred,
                                             const double* __restrict__ w1, const double* __restrict__ w2, int64_t p, int M) {
    if (a.method == SUSHI_HIP_METHOD_CCOEFF_NORMED)
        return centred ? score_ccoeff_at(corr_c_or_u, ts, a.centre, w1, w2, p, M)
                       : finish_ccoeff_normed(corr_c_or_u, w1[p + M] - w1[p], w2[p + M] - w2[p], ts, M);
    return centred ? score_at(corr_c_or_u, ts, a.centre, w1, w2, p, M) : score_exact(corr_c_or_u, ts, w2, p, M);
}

// TM_CCOEFF_NORMED: whether position p needs the cross term (a flat pattern, or windows cv2 takes for flat, give their value from
// the prefix sums alone); positions outside [0, P) need nothing
__device__ __forceinline__ bool needs_corr(const TileSrc& a, const TemplStats& ts, const double* __restrict__ w1,
                                           const double* __restrict__ w2, int64_t p, int P, int M) {
    const bool valid = p >= 0 && p < P;
    if (a.method != SUSHI_HIP_METHOD_CCOEFF_NORMED) return valid;
    return valid && !ccoeff_ignores_corr(w1[p + M] - w1[p], w2[p + M] - w2[p], ts, M);
}

// ------------------------------------------------------------------------------------------------------------------------
// uint8: Toeplitz GEMM on the i8 matrix pipe.  Positions p = p0 + 32 i + j of one 1024-position tile,
//     D[i][j] = sum_n A[i][n] B[n][j],   A[i][n] = T'[n - 32 i] (0 outside [0, M)),   B[n][j] = I'[win_start + p0 + j + n],
// n in [0, M + 992): K steps of 32.  T' = T - 128, I' = I - 128 as int8: the byte x ^ 0x80.
// Lane l (r = l & 31, h = l >> 5) holds A[r][32 s + 16 h + e] and B[32 s + 16 h + e][r], e = 0..15, in the bytes of its two
// 4-dword operands; C/D: column r, row (reg & 3) + 8 (reg >> 2) + 4 h (the same for every input type).  Whatever
// order the instruction gives the 32 k of a step inside a lane's 16 bytes, A and B are staged with the SAME k at the same byte,
// so the sum over k -- of integers, exact -- does not depend on it; row and column maps are checked bitwise by the GPU tests.
// The four waves of a workgroup take a quarter of the K steps each; their partial sums meet in LDS (integers: any order).
//
// Exactness (the proof obligation): every product is at most 2^14 in magnitude, so an int32 accumulator stays exact for
// 2^17 / 32 = 4096 steps; it is folded into float64 every FOLD_STEPS < 4096.  |sum T'I'| <= 2^14 M < 2^45 for any int32 M, so
// the float64 folds add integers below 2^53: exact.  score_at then forms sum T*I = corr_c + 128 (sum T + sum I) - 128^2 M,
// every term and partial sum an integer below 2^53 (sum T, sum I <= 255 M < 2^39): exact again -- the same integer the exact
// stages' float64 chain of uint8 products reaches (its partial sums are integers below 2^47: exact).  Equal cross terms through
// the same finish_* give the same float32.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int U8_TILE = 1024;
constexpr int FOLD_STEPS = 1024;        // 32,768 pattern samples per int32 chain (< 4096 steps: no overflow)

struct __attribute__((packed, aligned(1))) Bytes16 { uint8_t v[16]; };

// 16 centred samples x[k .. k + 16) of a row whose valid part is [lo, hi): the others are 0
__device__ __forceinline__ i32x4 load_centred16(const uint8_t* __restrict__ row, int64_t k, int64_t lo, int64_t hi) {
    i32x4 r;
    if (k >= lo && k + 16 <= hi) {
        const Bytes16 b = *reinterpret_cast<const Bytes16*>(row + k);
        memcpy(&r, &b, 16);
        r ^= (i32x4){(int)0x80808080, (int)0x80808080, (int)0x80808080, (int)0x80808080};
    } else {
        unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t x = k + e;
            if (x >= lo && x < hi) w[e >> 2] |= (unsigned)(row[x] ^ 0x80u) << (8 * (e & 3));
        }
        r = (i32x4){(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
    }
    return r;
}

// One tile of U8_TILE positions p0 .. p0 + 1023 (p0 may be negative: positions outside [0, P) are skipped), 256 threads.
// part: [4][U8_TILE] doubles of LDS, free when this is called (a barrier since its last use) and in use when it returns.
template <class Emit>
__device__ __forceinline__ void u8_tile(const TileSrc& a, const TileReq& d, int64_t p0, double (*part)[U8_TILE], Emit&& emit) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;
    const uint8_t* __restrict__ dst = (const uint8_t*)a.dst_raw;
    const uint8_t* __restrict__ src = (const uint8_t*)a.src_raw;
    const int M = d.M, P = d.P;
    const TemplStats ts = templ_stats(a.src_s1, a.src_s2, d.tmpl_off, M, a.centre);
    const double* __restrict__ w1 = a.dst_s1 + d.win_start;
    const double* __restrict__ w2 = a.dst_s2 + d.win_start;
    int need = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) need |= needs_corr(a, ts, w1, w2, p0 + tid + 256 * q, P, M);
    const bool any = __syncthreads_or(need) != 0;              // (uniform)

    double acc2[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc2[e] = 0.0;
    if (any) {
        const int steps = (M + 32 * 31 + 31) / 32;
        const int s_lo = (int)((int64_t)steps * wave / 4), s_hi = (int)((int64_t)steps * (wave + 1) / 4);
        const uint8_t* __restrict__ trow = src + d.tmpl_off;
        const int64_t g0 = d.win_start + p0 + r + 16 * h;      // dst sample of B's byte 0 at step 0 (>= 0: an absolute position)
        const int64_t t0 = 16 * h - 32 * r;                    // pattern sample of A's byte 0 at step 0
        for (int f0 = s_lo; f0 < s_hi; f0 += FOLD_STEPS) {
            const int f1 = min(s_hi, f0 + FOLD_STEPS);
            i32x16 acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0;
            i32x4 A = load_centred16(trow, t0 + 32 * (int64_t)f0, 0, M);
            i32x4 B = load_centred16(dst, g0 + 32 * (int64_t)f0, 0, a.dst_len);
            for (int s = f0; s < f1; ++s) {
                // the next step's operands are requested before this step's product (the last step re-requests its own)
                const int sn = s + 1 < f1 ? s + 1 : s;
                const i32x4 An = load_centred16(trow, t0 + 32 * (int64_t)sn, 0, M);
                const i32x4 Bn = load_centred16(dst, g0 + 32 * (int64_t)sn, 0, a.dst_len);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, B, acc, 0, 0, 0);
                A = An; B = Bn;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) acc2[e] += (double)acc[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) part[wave][32 * ((e & 3) + 8 * (e >> 2) + 4 * h) + r] = acc2[e];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = tid + 256 * q;
        const int64_t p = p0 + i;
        if (p >= 0 && p < P) {
            const double corr_c = ((part[0][i] + part[1][i]) + part[2][i]) + part[3][i];   // integers: exact in any order
            emit(i, p, curve_value(a, ts, corr_c, true, w1, w2, p, M));
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// float32: the canonical chain.  sum T*I over the samples as they are, in float64, XM pattern samples at a time: each chunk
// summed sequentially from its first sample, one fused multiply-add per sample, the chunk sums added in chunk order (the order
// sushi_exact.hip's exact stages keep).  A tile is 256 NPOS consecutive positions; a thread owns NPOS consecutive ones,
// which share its loads: at every sample the NPOS window values it needs are the previous sample's shifted by one.  XG chunks
// of the pattern and the window samples under them are staged in LDS as float64 at a time.
// ------------------------------------------------------------------------------------------------------------------------
constexpr int XM = 512;           // pattern samples per chunk of the canonical sum (sushi_exact.hip XM)
constexpr int XG = 4;             // chunks staged together
template <int NPOS> constexpr int f32_li_doubles() { return 256 * NPOS + XG * XM + (256 * NPOS + XG * XM) / 32 + 1; }

// One tile of 256 NPOS positions from p0 on (p0 may be negative: positions outside [0, P) are skipped), 256 threads.
// lt: [XG XM] and li: [f32_li_doubles<NPOS>()] doubles of LDS, free when this is called.
template <int NPOS, class Emit>
__device__ __forceinline__ void f32_tile(const TileSrc& a, const TileReq& d, int64_t p0, double* lt, double* li, Emit&& emit) {
    constexpr int SPAN = 256 * NPOS;
    const int tid = threadIdx.x;
    const float* __restrict__ dst = (const float*)a.dst_raw;
    const float* __restrict__ src = (const float*)a.src_raw;
    // window samples are staged with one padding element every 32: lanes NPOS samples apart then spread over the banks
    auto sk = [](const int e) { return e + (e >> 5); };
    const int M = d.M, P = d.P;
    const int n_chunks = (M + XM - 1) / XM;
    const TemplStats ts = templ_stats(a.src_s1, a.src_s2, d.tmpl_off, M, a.centre);
    const double* __restrict__ w1 = a.dst_s1 + d.win_start;
    const double* __restrict__ w2 = a.dst_s2 + d.win_start;
    const float* __restrict__ Tp = src + d.tmpl_off;
    const int64_t ibase = d.win_start + p0;                    // dst sample under position p0, pattern sample 0 (>= 0: absolute)
    int need = 0;
#pragma unroll
    for (int q = 0; q < NPOS; ++q) need |= needs_corr(a, ts, w1, w2, p0 + NPOS * tid + q, P, M);
    const bool any = __syncthreads_or(need) != 0;              // (uniform)
    double tot[NPOS];
#pragma unroll
    for (int q = 0; q < NPOS; ++q) tot[q] = 0.0;
    for (int c0 = 0; any && c0 < n_chunks; c0 += XG) {
        const int m0 = c0 * XM;
        const int gm = min(XG * XM, M - m0);                   // pattern samples of this group
        __syncthreads();                                       // the previous group's reads are done
        for (int e = tid; e < gm; e += 256) lt[e] = (double)Tp[m0 + e];
        const int wn = SPAN + gm - 1;                          // window samples the group's positions read
        for (int e = tid; e < wn; e += 256) {
            const int64_t g = ibase + m0 + e;
            li[sk(e)] = g < a.dst_len ? (double)dst[g] : 0.0;
        }
        __syncthreads();
        for (int c = 0; c < XG && m0 + c * XM < M; ++c) {
            const int mb = c * XM;                             // chunk start inside the staged group
            const int mc = min(XM, M - m0 - mb);
            double acc[NPOS];
            double w[NPOS];
#pragma unroll
            for (int q = 0; q < NPOS; ++q) { acc[q] = 0.0; w[q] = li[sk(NPOS * tid + mb + q)]; }
            for (int m = 0; m < mc; ++m) {
                const double t = lt[mb + m];
#pragma unroll
                for (int q = 0; q < NPOS; ++q) acc[q] = __builtin_fma(t, w[q], acc[q]);
                // slide: position q's next window sample is position q + 1's current one
#pragma unroll
                for (int q = 0; q + 1 < NPOS; ++q) w[q] = w[q + 1];
                w[NPOS - 1] = li[sk(NPOS * tid + mb + m + NPOS)];
            }
#pragma unroll
            for (int q = 0; q < NPOS; ++q) tot[q] += acc[q];   // chunk sums in chunk order
        }
    }
#pragma unroll
    for (int q = 0; q < NPOS; ++q) {
        const int i = NPOS * tid + q;
        const int64_t p = p0 + i;
        if (p >= 0 && p < P) emit(i, p, curve_value(a, ts, tot[q], false, w1, w2, p, M));
    }
}

}  // namespace sushi_tiles
#endif
