// sushi_amd/csrc/sushi_direct.hip -- gfx950 (MI355X, CDNA4): the direct path of Sushi's audio template match, one MFMA kernel.
//
// Replaces, for a whole batch of (pattern, window) pairs, what the reference does per call in
//   wav.py:185  result = cv2.matchTemplate(search_source, pattern, cv2.TM_SQDIFF_NORMED)
//   wav.py:186  min_idx = result.argmin(axis=1)[0]
// i.e. R[p] = sum_m (T[m]-I[p+m])^2 / sqrt(sum T^2 * sum_m I[p+m]^2) with OpenCV's clamp, then first argmin.
//
// Formulation (DESIGN.md "Kernel K1"):
//   * streams are stored centred (xc = x - c, c = 0.5 | 128) so the cross term is small and the
//     sum-of-squares identity  sum (T-I)^2 = sum T'^2 - 2 sum T'I' + sum I'^2  loses nothing;
//     sum T'^2, sum I'^2, sum T', sum I' come from float64 prefix arrays built once per stream.
//   * the sliding dot product corr[p] = sum_m T'[m] I'[p+m] is computed as a GEMM with one
//     Toeplitz operand, on the exact-f32 matrix pipe (v_mfma_f32_32x32x2_f32):
//         p = base + 32 i + j ,   D[i][j] += sum_n A[i][n] B[n][j]
//         A[i][n] = T'[n - 32 i]  (zero outside [0,M))      B[n][j] = I'[base + j + n]
//     One MFMA tile therefore owns 1024 consecutive positions.  A is read from an LDS copy of
//     the template chunk laid out with a +1 skew every 32 floats (lane stride 33 -> no bank
//     conflict), B from a plain contiguous LDS copy of the search tile (lane stride 1).
//   * f32 accumulation is restarted every FLUSH template samples and folded into float64
//     accumulators, so the error of the f32 chains stays below cv2's own float32 quantum of corr.
//   * epilogue: OpenCV common_matchTemplate() in float64, result rounded to float32, packed with
//     the position into a 64-bit key; wave shuffles + LDS + one atomicMin per workgroup give the
//     first-index argmin (NumPy argmin semantics).
//
// gfx950 only: wave64, 4 SIMDs/CU, 160 KiB LDS/CU.  No CUDA compatibility paths.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>

#include "../../include/sushi_hip.h"
#include "sushi_common.hpp"
#include "sushi_internal.hpp"

namespace {

using namespace sushi;

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KC = 512;          // template samples per LDS chunk
constexpr int FLUSH = 128;       // length of one f32 accumulation chain before it is folded into float64
constexpr int ROWSPAN = 32 * 31; // 992: largest row shift 32*i of the Toeplitz operand
constexpr int TLEN = KC + ROWSPAN;              // template samples staged per chunk
constexpr int TLDS = TLEN + TLEN / 32 + 1;      // with the +1-per-32 skew

struct MatchArgs {
    const float* dst_xc;
    const double* dst_s1;
    const double* dst_s2;
    int64_t dst_len;
    const float* src_xc;
    const double* src_s1;
    const double* src_s2;
    int64_t src_len;
    double centre;
    const SearchDesc* searches;
    int n_search;
    int n_tiles;
    int method;                   // SUSHI_HIP_METHOD_*
    unsigned long long* keys;
};

template <int WAVES, int NB> struct TileShape {
    static constexpr int NT = WAVES * 64;
    static constexpr int TP = WAVES * NB * 1024;        // positions per workgroup
    static constexpr int ILEN = TP + KC - 984;          // search samples staged per chunk: TP-1024+32 columns + KC rows + align slack, multiple of 4
    static constexpr int LDS_FLOATS = ILEN + TLDS;
};

// One tile (TP consecutive result positions) of one search.  `lds` holds LDS_FLOATS floats, `red` WAVES keys.
template <int WAVES, int NB>
__device__ __forceinline__ void match_tile(const MatchArgs& a, const int s_idx, const SearchDesc sd,
                                           const int tile_in_search, float* lds, unsigned long long* red) {
    constexpr int NT = TileShape<WAVES, NB>::NT;
    constexpr int TP = TileShape<WAVES, NB>::TP;
    constexpr int ILEN = TileShape<WAVES, NB>::ILEN;
    float* I_lds = lds;
    float* T_lds = lds + ILEN;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31;                     // MFMA row (A) / column (B) index of this lane
    const int h = lane >> 5;                     // MFMA k index of this lane

    const int M = sd.tmpl_len;
    const int P = sd.n_pos;
    const int p0 = tile_in_search * TP;          // first position of this workgroup
    const int wb = wave * (NB * 1024);           // first position of this wave inside the tile
    const bool wave_active = (p0 + wb) < P;

    const float* __restrict__ src = a.src_xc + sd.tmpl_off;
    const int64_t gwin = sd.win_start + p0;      // dst sample under position p0, template sample 0

    f32x16 acc[NB];
    double acc2[NB][16];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[b][r] = 0.f; acc2[b][r] = 0.0; }
    }

    const int nchunks = (M + ROWSPAN + KC - 1) / KC;
    for (int c = 0; c < nchunks; ++c) {
        const int n1 = c * KC;
        // ---- stage the search tile: dst[gwin + n1 .. + TP + KC) as aligned float4 ---------
        const int64_t g = gwin + n1;
        const int64_t gA = g & ~(int64_t)3;
        const int ioff = (int)(g - gA);
        __syncthreads();                          // previous chunk's LDS reads are done
        for (int v = tid; v < ILEN / 4; v += NT) {
            const int64_t e = gA + 4 * (int64_t)v;
            float4 val;
            if (e + 3 < a.dst_len) {
                val = *reinterpret_cast<const float4*>(a.dst_xc + e);
            } else {
                val.x = (e + 0 < a.dst_len) ? a.dst_xc[e + 0] : 0.f;
                val.y = (e + 1 < a.dst_len) ? a.dst_xc[e + 1] : 0.f;
                val.z = (e + 2 < a.dst_len) ? a.dst_xc[e + 2] : 0.f;
                val.w = 0.f;
            }
            *reinterpret_cast<float4*>(I_lds + 4 * v) = val;
        }
        // ---- stage the template chunk T'[n1-992 .. n1+KC), zero outside [0,M), skewed ------
        for (int y = tid; y < TLEN; y += NT) {
            const int x = n1 - ROWSPAN + y;
            const float v = (x >= 0 && x < M) ? src[x] : 0.f;
            T_lds[y + (y >> 5)] = v;
        }
        __syncthreads();

        if (wave_active) {
            const float* tp = T_lds + (h + 33 * (31 - i));
            const float* ip = I_lds + (ioff + wb + i + h);
            for (int nf = 0; nf < KC; nf += FLUSH) {
                // FLUSH/4 groups of two k-steps (= 4 template samples, 2*NB MFMAs).  The operands of
                // group g+1 are read from LDS before the MFMAs of group g are issued (register
                // double buffer); sched_group_barrier pins that order so the matrix pipe never waits
                // on an LDS round trip.
                const float* tq = tp + nf + (nf >> 5);
                const float* iq = ip + nf;
                float a_cur[2], b_cur[NB][2], a_nxt[2], b_nxt[NB][2];
                a_cur[0] = tq[0]; a_cur[1] = tq[2];
#pragma unroll
                for (int b = 0; b < NB; ++b) { b_cur[b][0] = iq[1024 * b]; b_cur[b][1] = iq[1024 * b + 2]; }
#pragma unroll
                for (int g = 0; g < FLUSH / 4; ++g) {
                    if (g + 1 < FLUSH / 4) {
                        const int n = 4 * (g + 1);                   // offset inside the flush block
                        const int tn = n + (n >> 5);                 // skewed template offset (nf % 32 == 0)
                        a_nxt[0] = tq[tn]; a_nxt[1] = tq[tn + 2];
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            b_nxt[b][0] = iq[n + 1024 * b]; b_nxt[b][1] = iq[n + 1024 * b + 2];
                        }
                        __builtin_amdgcn_sched_group_barrier(0x100, NB + 1, 0);   // DS reads of group g+1
                    }
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
#pragma unroll
                        for (int b = 0; b < NB; ++b)
                            acc[b] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur[k], b_cur[b][k], acc[b], 0, 0, 0);
                    }
                    __builtin_amdgcn_sched_group_barrier(0x8, 2 * NB, 0);         // MFMAs of group g
                    if (g + 1 < FLUSH / 4) {
                        a_cur[0] = a_nxt[0]; a_cur[1] = a_nxt[1];
#pragma unroll
                        for (int b = 0; b < NB; ++b) { b_cur[b][0] = b_nxt[b][0]; b_cur[b][1] = b_nxt[b][1]; }
                    }
                }
                // fold the f32 chain (FLUSH products long) into the float64 accumulators
#pragma unroll
                for (int b = 0; b < NB; ++b) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) { acc2[b][r] += (double)acc[b][r]; acc[b][r] = 0.f; }
                }
            }
        }
    }

    // ---- epilogue: normalise, pack (score, position), arg-min ------------------------------
    unsigned long long best = ~0ull;
    if (wave_active) {
        const TemplStats ts = templ_stats(a.src_s1, a.src_s2, sd.tmpl_off, M, a.centre);
        const double* __restrict__ w1 = a.dst_s1 + sd.win_start;
        const double* __restrict__ w2 = a.dst_s2 + sd.win_start;
#pragma unroll
        for (int b = 0; b < NB; ++b) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // C/D layout of 32x32 MFMA: col = lane & 31, row = (r&3) + 8*(r>>2) + 4*(lane>>5)
                const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int p = p0 + wb + 1024 * b + 32 * row + i;
                if (p < P) {
                    const unsigned long long key = a.method == SUSHI_HIP_METHOD_CCOEFF_NORMED
                        ? make_key_max(score_ccoeff_at(acc2[b][r], ts, a.centre, w1, w2, p, M), (unsigned)p)
                        : make_key(score_at(acc2[b][r], ts, a.centre, w1, w2, p, M), (unsigned)p);
                    best = key < best ? key : best;
                }
            }
        }
    }
    best = wave_min_u64(best);
    if (lane == 0) red[wave] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = red[0];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) m = red[w] < m ? red[w] : m;
        if (m != NO_KEY) atomicMin(a.keys + s_idx, m);
    }
}


template <int WAVES, int NB>
__global__ __launch_bounds__(WAVES * 64, 2)
void match_sqdiff_f32_kernel(MatchArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[TileShape<WAVES, NB>::LDS_FLOATS];
    __shared__ unsigned long long red[WAVES];
    // ---- which search / which tile ------------------------------------------------------
    const int tile = xcd_remap(blockIdx.x, a.n_tiles);
    int lo = 0, hi = a.n_search - 1;             // last search with first_tile <= tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.searches[mid].first_tile <= tile) lo = mid; else hi = mid - 1;
    }
    const SearchDesc sd = a.searches[lo];
    match_tile<WAVES, NB>(a, lo, sd, tile - sd.first_tile, lds, red);
}

struct Variant { int waves, nb; };
constexpr Variant kVariants[] = {{1, 1}, {4, 1}, {4, 4}};
constexpr int kNumVariants = 3;

}  // namespace

namespace sushi {

int direct_variant_count() { return kNumVariants; }

int direct_variant_tile(int variant) {
    if (variant < 0 || variant >= kNumVariants) return 0;
    return kVariants[variant].waves * kVariants[variant].nb * 1024;
}

int launch_direct(const StreamRefs& r, const SearchDesc* searches_dev, int n_search, int n_tiles, int variant, int method,
                  unsigned long long* keys_dev, int32_t* out_idx_dev, float* out_score_dev, int32_t* out_packed_dev, hipStream_t st) {
    if (n_tiles < n_search || variant < 0 || variant >= kNumVariants) return SUSHI_HIP_EINVAL;
    if (!method_known(method)) return SUSHI_HIP_EINVAL;
    if (hipMemsetAsync(keys_dev, 0xff, (size_t)n_search * sizeof(uint64_t), st) != hipSuccess) return SUSHI_HIP_ELAUNCH;
    MatchArgs a;
    a.dst_xc = r.dst_xc; a.dst_s1 = r.dst_s1; a.dst_s2 = r.dst_s2; a.dst_len = r.dst_len;
    a.src_xc = r.src_xc; a.src_s1 = r.src_s1; a.src_s2 = r.src_s2; a.src_len = r.src_len;
    a.centre = r.centre; a.searches = searches_dev; a.n_search = n_search; a.n_tiles = n_tiles;
    a.keys = keys_dev; a.method = method;
    switch (variant) {
        case 0: hipLaunchKernelGGL((match_sqdiff_f32_kernel<1, 1>), dim3(n_tiles), dim3(64), 0, st, a); break;
        case 1: hipLaunchKernelGGL((match_sqdiff_f32_kernel<4, 1>), dim3(n_tiles), dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((match_sqdiff_f32_kernel<4, 4>), dim3(n_tiles), dim3(256), 0, st, a); break;
    }
    if (launch_ok() != SUSHI_HIP_OK) return SUSHI_HIP_ELAUNCH;
    return launch_unpack(keys_dev, n_search, method, out_idx_dev, out_score_dev, out_packed_dev, st);
}

}  // namespace sushi
