// sushi_amd/csrc/sushi_fft_store.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// packed-half storage: scales, the order spectra are stored in, the low band of a row and the norms outside it.

// ---- block spectra, pattern spectra and their products Y are all kept as packed halves -----------------------------
// (half the bytes of everything the step moves between kernels, and two multiply-adds per v_dot2_f32_f16 in mac_kernel)
// Two things make 11 bits enough for a stage that only ranks:
//  * block spectra are of the CENTRED destination samples (x - c), patterns stay as they are:
//        y'[p] = sum_m T[m] (I[p+m] - c) = sum T I - c sum T
//    -- the correction is one constant per search -- and Y then carries no product of two DC terms: its energy, and with
//    it the quantisation noise of every position, is that of pattern x centred audio instead of ~M/4 at every position;
//  * the noise is modelled per pair from the energy of the Y row actually loaded (Parseval), added to the pair's error
//    bound, and checked like the rest of the bound (candidates and one audited non-candidate per search, refine_kernel).
//    Rounding the two factors to halves before they are multiplied perturbs a product Tt_s(f) Z_j(f) by the same relative
//    2^-11 per factor as rounding the sum does afterwards: with the terms of a bin's sum taken as independent that is two
//    more times the variance of the stored row's own rounding (pair_error_model).
// The constant c is the stream's own mean (any constant is exact; the mean keeps DC out whatever level the data sits at).
// Power-of-two scales keep every stored half inside the format whatever the magnitude of the data, and away from its
// subnormals: block spectra by the stream (|Z_j(f)| <= sqrt(2 N E7), E7 = the largest centred energy of FFT_STEP + 1
// consecutive blocks, SushiHipStream.stats), pattern spectra by the pattern (|Tt_s(f)| <= 64 |T| / N), and the float32
// sums of their products are brought to the scale of Y when they are stored:
//   |Y(f)| <= sum_s |Tt_s(f)| * max_j |Z_j(f)| <= (64 sqrt(n_seg) |T| / N) * (sqrt(7 * 4096) sqrt(E7));
// typical values sit ~sqrt(N) below these bounds, twenty binary orders above the smallest normal half.
__device__ __forceinline__ float pow2_under(double target, double bound) {
    if (!(bound > 0.0)) return 1.0f;
    int k = (int)floor(log2(target / bound));
    k = k < -60 ? -60 : (k > 60 ? 60 : k);
    return (float)ldexp(1.0, k);
}
__device__ __forceinline__ float y_scale_for(double tnorm, int n_seg, double e7) {
    return pow2_under(32768.0, (64.0 * sqrt((double)n_seg) * tnorm / (double)FN) * (169.33 * sqrt(e7)));
}
__device__ __forceinline__ float z_scale_for(double e7) { return pow2_under(32768.0, 181.02 * sqrt(e7)); }
__device__ __forceinline__ float t_scale_for(double tnorm) { return pow2_under(8192.0, 64.0 * tnorm / (double)FN); }
// one complex number as a packed half pair (re | im << 16), round to nearest even, never infinite
__device__ __forceinline__ unsigned pack_h2(float re, float im) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 q = {(_Float16)__builtin_amdgcn_fmed3f(re, -65504.f, 65504.f), (_Float16)__builtin_amdgcn_fmed3f(im, -65504.f, 65504.f)};
    return __builtin_bit_cast(unsigned, q);
}
// sum of |re|^2 + |im|^2 over the four stored words (re | im << 16) of one 16-byte entry, added to `acc`.
// The entry is cast to EIGHT halves as a whole and taken apart by sub-vectors: hipcc 7.2 compiles the obvious form --
// `bit_cast<half2>(entry[j])` for j = 0 .. 3 in an unrolled loop -- to four reads of the entry's FIRST word (it narrows the 16-byte
// load to a dword: `v_dot2c_f32_f16 v7, v2, v2` four times over; a ten-line reproducer is in tools/experiments/README.md).  The row
// energies behind the error model were therefore four times every fourth bin: right on noise-like rows, a factor 10^4 short on
// a row whose energy sits in one bin.  Found in round 6 with bursts of a tone (tests/test_bound_stress.py "fs8burst").
__device__ __forceinline__ float add_abs2_entry(const sushi_fft::uint4v e, float acc) {
    typedef _Float16 h8 __attribute__((ext_vector_type(8)));
    const h8 v = __builtin_bit_cast(h8, e);
    acc = __builtin_amdgcn_fdot2(v.s01, v.s01, acc, false);
    acc = __builtin_amdgcn_fdot2(v.s23, v.s23, acc, false);
    acc = __builtin_amdgcn_fdot2(v.s45, v.s45, acc, false);
    return __builtin_amdgcn_fdot2(v.s67, v.s67, acc, false);
}
static_assert(ROWE == FN / sushi_mac::BINS && LROWE == sushi_fft::LB_ENTRIES, "sushi_geometry.hpp's rows are mac_core's lanes and fft_core's low band");
constexpr float Y_KQ = 8.0f;                  // the quantisation term of a pair's bound, in standard deviations
static_assert(FFT_LOGN == 14 && sushi_fft::W_LDS_FLOATS <= LDS_FLOATS && FT == sushi_fft::WNT, "the wave plan is the 16384-point inverse");

// Spectra are STORED in the order the inverse transform loads them (fft_core.hpp "Wave plan": wslot_of_bin): block
// spectra, pattern spectra and their products only have to agree on one order of the bins.  A forward transform ends with
// thread tid holding X[tid + 1024 r] in register r.
// That is a permutation of the THREADS (same register index): the bins register r of thread (w, l) loads are held, after
// a forward transform, by register r of thread w + 64 (l & 15) + 16 (l >> 4).  The forward kernels hand their outputs
// over through the LDS (real parts, then imaginary parts; position tid + tid / 64 makes the gather conflict-free) so that
// the global stores are whole KiB per wave instead of 16-byte pieces 8 KiB apart (pattern spectra are written every run).
__device__ __forceinline__ void to_load_order(cpx (&v)[sushi_fft::PER], const int tid, float* lds) {
    // element e of the stored order sits at e + e / 16 + e / 1024 (the producer's scattered stores then spread over the banks);
    // a thread takes its four runs of four (the entries it will store) back out
    auto pos = [](const int e) { return e + (e >> 4) + (e >> 10); };
    __syncthreads();                                             // the transform's own use of the buffer is over
#pragma unroll
    for (int r = 0; r < sushi_fft::PER; ++r) lds[pos(sushi_fft::mslot_of_bin(tid + FT * r))] = v[r].x;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < sushi_fft::PER; ++r) v[r].x = lds[pos(4 * sushi_fft::wslot_uint4(tid, r >> 2) + (r & 3))];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < sushi_fft::PER; ++r) lds[pos(sushi_fft::mslot_of_bin(tid + FT * r))] = v[r].y;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < sushi_fft::PER; ++r) v[r].y = lds[pos(4 * sushi_fft::wslot_uint4(tid, r >> 2) + (r & 3))];
}
static_assert(FN + FN / 16 + FN / 1024 <= LDS_FLOATS, "the hand-over fits the transform's buffer");

// exp(-2*pi*i*n/16384), n = 0..16383, float32 rounded from float64 (generated by sushi_amd/build.py)
__device__ const float g_twiddle[2 * sushi_fft::TWIDDLE_N] = {
#include "_gen_twiddle16384.inc"
};

__device__ __forceinline__ const cpx* twiddles() { return reinterpret_cast<const cpx*>(g_twiddle); }

// B operands of the inverse transform's first pass on the matrix pipe: [product][lane] x 8 halves (generated by sushi_amd/build.py)
__device__ __attribute__((aligned(16))) const unsigned g_dft16_b[4 * 64 * 4] = {
#include "_gen_dft16_f16.inc"
};
__device__ __forceinline__ sushi_fft::MfmaB dft16_operands(const int tid) {
    return sushi_fft::load_mfma_b(tid, reinterpret_cast<const sushi_fft::uint4v*>(g_dft16_b));
}
// ... and of bound_kernel's first pass: the matrix's high halves times 2^-10 (generated by sushi_amd/build.py)
__device__ __attribute__((aligned(16))) const unsigned g_dft16_bh[2 * 64 * 4] = {
#include "_gen_dft16_f16_bound.inc"
};

// ... and of bound_low_kernel's (K = 16: the eight d1 a low-band group holds; generated by sushi_amd/build.py)
__device__ __attribute__((aligned(16))) const unsigned g_dft16_bl[2 * 64 * 2] = {
#include "_gen_dft16_f16_bound_low.inc"
};

// What a forward transform leaves for the band-split exclusion.  Thread tid ends with X[tid + 1024 r] in register r: the low band
// is r = 0, 1, 14, 15 of every thread -- one 16-byte entry of the low row (fft_core.hpp lslot_of_thread) --, and of the other
// twelve bins the energy of the halves AS STORED is summed: |sum over the bins outside the band of Tt_s(f) Z_j(f)| is at most
// the product of the two rows' norms outside the band (Cauchy-Schwarz), whatever the phases.
// The band is kept MIRROR-SYMMETRIC: bin 7N/8 (thread 0's register 14) has its mirror N/8 outside the band, so it is counted with
// the rest -- its low-row entry is zero and its energy goes to the norm -- and the band is |f| < N/8 strictly.  slb_kernel's split
// of the rest into the two real blocks' parts (real_block_rest_norms) holds over a mirror-symmetric set of bins only (ADVICE r5).
__device__ __forceinline__ uint4 low_entry_and_rest(const cpx (&v)[sushi_fft::PER], const float sc, const int tid, float& rest2) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    float e = 0.f;
#pragma unroll
    for (int r = 2; r < 14; ++r) {
        const h2 h = __builtin_bit_cast(h2, pack_h2(v[r].x * sc, v[r].y * sc));
        e = __builtin_amdgcn_fdot2(h, h, e, false);
    }
    unsigned e14 = pack_h2(v[14].x * sc, v[14].y * sc);
    if (tid == 0) {
        const h2 h = __builtin_bit_cast(h2, e14);
        e = __builtin_amdgcn_fdot2(h, h, e, false);
        e14 = 0u;
    }
    rest2 = e;
    return uint4{pack_h2(v[0].x * sc, v[0].y * sc), pack_h2(v[1].x * sc, v[1].y * sc), e14, pack_h2(v[15].x * sc, v[15].y * sc)};
}
// the low entries of a workgroup into their row (whole KiB per wave through the LDS) and the norm of the rest (red: FT / 64 floats)
__device__ __forceinline__ float wave_sum_shfl(float w) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) w += __shfl_xor(w, d, 64);
    return w;
}
__device__ __forceinline__ void store_low_row(const uint4 low, const float rest2, const int tid, float* lds, float* red,
                                              uint4* __restrict__ low_row, float* __restrict__ norm_out) {
    const float w = wave_sum_shfl(rest2);
    __syncthreads();                                             // the hand-over's use of the buffer is over
    uint4* l4 = reinterpret_cast<uint4*>(lds);
    // (one entry of padding per 128: the eight groups a wave's lanes scatter to are then eight different banks)
    const int pos = sushi_fft::lslot_of_thread(tid);
    l4[pos + (pos >> 7)] = low;
    if ((tid & 63) == 0) red[tid >> 6] = w;
    __syncthreads();
    low_row[tid] = l4[tid + (tid >> 7)];
    if (tid == 0) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < FT / 64; ++i) t += red[i];
        *norm_out = sqrtf(t) * 1.000002f;
    }
}
// A block spectrum packs TWO real blocks, Z = A + i B (A, B the conjugate-symmetric spectra of the real blocks at j B and
// j B + H): the real parts of a pair's transform outputs come from A alone, the imaginary parts from B alone, and
// |A|^2 + |B|^2 = |Z|^2 over a symmetric set of bins -- so bounding the two parts separately, each from its own block's norm,
// saves the factor sqrt(2) a bound from |Z| pays.  A(f) = (Z(f) + conj Z(N - f)) / 2, B(f) = (Z(f) - conj Z(N - f)) / 2i, of the
// halves AS STORED; bin N - f of thread tid's register r is register 15 - r of thread FT - tid (tid > 0; tid 0: register
// (16 - r) % 16 of itself).  out[0 / 1] = the norms of A / B over the bins outside the band.
__device__ __forceinline__ void real_block_rest_norms(const cpx (&v)[sushi_fft::PER], const float sc, const int tid, float* lds,
                                                      float* red, float* __restrict__ out_a, float* __restrict__ out_b) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    unsigned* w = reinterpret_cast<unsigned*>(lds);
    __syncthreads();
#pragma unroll
    for (int r = 1; r < 15; ++r) w[(r - 1) * FT + tid] = pack_h2(v[r].x * sc, v[r].y * sc);   // (registers 1 and 14: tid 0's partners of 15 and 2 are not needed; kept simple)
    __syncthreads();
    const int pt = tid == 0 ? 0 : FT - tid;
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int r = 2; r < 14; ++r) {
        const int pr = tid == 0 ? 16 - r : 15 - r;                  // 2 .. 13 -> 13 .. 2 (tid > 0), 14 .. 3 (tid 0)
        const h2 z = __builtin_bit_cast(h2, pack_h2(v[r].x * sc, v[r].y * sc));
        const h2 m = __builtin_bit_cast(h2, w[(pr - 1) * FT + pt]);
        const float ar = (float)z.x + (float)m.x, ai = (float)z.y - (float)m.y;      // Z(f) + conj Z(N - f)
        const float br = (float)z.x - (float)m.x, bi = (float)z.y + (float)m.y;      // Z(f) - conj Z(N - f)
        // (bin 7N/8 -- thread 0's register 14, counted with the rest: low_entry_and_rest -- is the mirror of bin N/8, thread 0's
        // register 2: the same moduli once more)
        const float twice = tid == 0 && r == 2 ? 2.f : 1.f;
        sa += twice * (ar * ar + ai * ai);
        sb += twice * (br * br + bi * bi);
    }
    sa = wave_sum_shfl(sa); sb = wave_sum_shfl(sb);
    __syncthreads();
    if ((tid & 63) == 0) { red[tid >> 6] = sa; red[FT / 64 + (tid >> 6)] = sb; }
    __syncthreads();
    if (tid == 0) {
        float ta = 0.f, tb = 0.f;
#pragma unroll
        for (int i = 0; i < FT / 64; ++i) { ta += red[i]; tb += red[FT / 64 + i]; }
        *out_a = sqrtf(0.25f * ta) * 1.000004f;
        *out_b = sqrtf(0.25f * tb) * 1.000004f;
    }
}
static_assert(LROWE == FT && LROW_BYTES + LROWE / 128 * 16 <= LDS_FLOATS * 4 && 14 * FT <= LDS_FLOATS, "one low entry per forward thread");
