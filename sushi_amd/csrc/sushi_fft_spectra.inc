// sushi_amd/csrc/sushi_fft_spectra.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// spectra_kernel (once per destination stream) and tspec_kernel (pattern segments, every run).

// ------------------------------------------------------------------------------------------
// Destination-stream spectra
// ------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(FT)
void spectra_kernel(const T* __restrict__ raw, int64_t n, uint32_t* __restrict__ spec, const double* __restrict__ stats,
                    uint4* __restrict__ spec_low, float* __restrict__ znorm_rest, const int64_t norm_stride) {
    const float centre = (float)stats[1];
    const float sz = z_scale_for(stats[0]);
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    __shared__ float red[2 * (FT / 64)];
    const int tid = threadIdx.x;
    const sushi_fft::Twiddles tw = sushi_fft::load_twiddles<FFT_LOGN, -1>(tid, twiddles());
    const int64_t j = blockIdx.x;
    const int64_t base = j * FFT_SEG;
    cpx v[sushi_fft::PER];
#pragma unroll
    for (int r = 0; r < sushi_fft::PER; ++r) {
        // unconditional loads from clamped addresses + select: the loads stay batched
        const int64_t e = base + sushi_fft::in_index<FFT_LOGN>(tid, r);
        const float xa = (float)raw[e < n ? e : n - 1] - centre;      // centred (above); zeros past the end of the stream
        const float xb = (float)raw[(e + FH) < n ? (e + FH) : n - 1] - centre;
        v[r].x = e < n ? xa : 0.f;
        v[r].y = (e + FH) < n ? xb : 0.f;
    }
    sushi_fft::fft_split<FFT_LOGN, -1>(v, tid, lds, tw);
    float rest2;
    const uint4 low = low_entry_and_rest(v, sz, tid, rest2);
    real_block_rest_norms(v, sz, tid, lds, red, znorm_rest + norm_stride + j, znorm_rest + 2 * norm_stride + j);
    to_load_order(v, tid, lds);
    uint4* __restrict__ out = reinterpret_cast<uint4*>(spec + (size_t)j * FN);
#pragma unroll
    for (int u = 0; u < sushi_fft::PER / 4; ++u)
        out[sushi_fft::wslot_uint4(tid, u)] = uint4{pack_h2(v[4 * u].x * sz, v[4 * u].y * sz), pack_h2(v[4 * u + 1].x * sz, v[4 * u + 1].y * sz),
                                                    pack_h2(v[4 * u + 2].x * sz, v[4 * u + 2].y * sz), pack_h2(v[4 * u + 3].x * sz, v[4 * u + 3].y * sz)};
    store_low_row(low, rest2, tid, lds, red, spec_low + (size_t)j * LROWE, znorm_rest + j);
}

// last search of [0, n) whose first_seg is <= x
__device__ __forceinline__ int find_search_by_seg(const SearchDesc* __restrict__ s, int n, int x) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (s[mid].first_seg <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------
// Pattern-segment spectra: Tt = conj(DFT(t_s zero padded)) / N, stored as the packed halves (Re Tt, -Im Tt) mac_kernel's
// dot products take (mac_core.hpp) -- the scaled forward transform itself.  The workgroup of a search's first
// segment also writes the search's scoring constants and the pair -> search map ifft_kernel reads.
// ------------------------------------------------------------------------------------------
struct TspecArgs {
    const void* src_raw;              // the source stream's samples as they are (uint8 or float32)
    const SearchDesc* searches;       // the sub-batch's searches
    int n_sub;
    int sub_first_seg;
    int sub_first_pair;
    uint32_t* tspec;                  // [segments of the sub-batch] packed halves: whole rows of FN words (tspec_kernel) or half rows of 4 HROWE (tspec_real_kernel)
    int* pairmap;                     // [pairs of the sub-batch] -> search index inside the sub-batch
    TemplConsts* tconst;      // [searches of the sub-batch]
    const double* src_s1;
    const double* src_s2;
    double centre;
    const double* dst_stats;          // the searched stream's stats: [0] largest energy of a pair's span, [1] its centring constant
    int method;                       // SUSHI_HIP_METHOD_CCOEFF_NORMED: spectra of the pattern minus its own mean
    uint4* tspec_low;                 // [segments of the sub-batch][LROWE] the low band again, in bound_low_kernel's order
    float* tnorm_rest;                // [segments of the sub-batch] SQUARED norm of the stored halves outside the band (accumulated: zero it first)
};

// What both routes of the kernel do first: find the segment's search, take the pattern's statistics and scales, and -- the
// workgroup of a search's first segment -- write the search's constants and its pairs' map.  NT: the workgroup's threads.
struct TspecSeg {
    int64_t off;                      // the segment's first sample in the source stream
    int len;                          // its samples (1 .. FFT_SEG)
    float t_sub;                      // what is subtracted from every sample (TM_CCOEFF_NORMED: the pattern's mean)
    float sc;                         // t_scale / N
};
template <int NT>
__device__ __forceinline__ TspecSeg tspec_segment(const TspecArgs& a, const int tid) {
    const int seg = a.sub_first_seg + blockIdx.x;
    const int k = find_search_by_seg(a.searches, a.n_sub, seg);
    const SearchDesc sd = a.searches[k];
    const int s = seg - sd.first_seg;
    const int M = sd.tmpl_len;
    const TemplStats ts_all = templ_stats(a.src_s1, a.src_s2, sd.tmpl_off, M, a.centre);
    // TM_CCOEFF_NORMED correlates the pattern MINUS ITS OWN MEAN: sum (T - mean T) I is that method's numerator as it is (no
    // window-sum term left to subtract, nothing of the pattern's level in the products), and what the spectra hold -- and the
    // scales are sized by -- is the centred pattern's norm.  (A pattern without variance is answered without its spectra.)
    const bool cc = a.method == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    const double tn_spec = cc && !ts_all.flat ? ts_all.tnorm_c : ts_all.tnorm;
    const float y_scale = y_scale_for(tn_spec, (M + FFT_SEG - 1) / FFT_SEG, a.dst_stats[0]);
    const float t_scale = t_scale_for(tn_spec);
    if (s == 0) {
        const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, M);
        int* __restrict__ pm = a.pairmap + first_pair_in_sub(a.sub_first_pair, sd);
        for (int i = tid; i < lay.n_pairs; i += NT) pm[i] = k;
        if (tid == 0) {
            const TemplStats ts = templ_stats(a.src_s1, a.src_s2, sd.tmpl_off, M, a.centre);
            TemplConsts tc;
            tc.tU = ts.tU; tc.inv_tnorm = (float)(1.0 / ts.tnorm); tc.tnorm = (float)ts.tnorm;
            tc.tmean = (float)ts.tmean; tc.flat = ts.flat ? 1 : 0;
            tc.inv_tnorm_c = ts.flat ? 0.f : (float)(1.0 / ts.tnorm_c); tc.inv_m = (float)(1.0 / (double)M);
            tc.c_sum_t = cc ? 0.f : (float)(a.dst_stats[1] * ts.tS1);      // (the centred pattern sums to zero)
            tc.inv_scale = 1.0f / y_scale;
            tc.mac_scale = (float)((double)y_scale / ((double)t_scale * (double)z_scale_for(a.dst_stats[0])));
            a.tconst[k] = tc;
        }
    }
    TspecSeg g;
    g.off = sd.tmpl_off + (int64_t)s * FFT_SEG;
    g.len = min(FFT_SEG, M - s * FFT_SEG);
    g.t_sub = cc ? (float)ts_all.tmean : 0.f;
    g.sc = t_scale / (float)FN;
    return g;
}

// The complex route (SUSHI_HIP_TSPEC=complex; the route of every run before the real one existed, kept for A/B measurements on
// one build): the zero-padded segment through a full 16384-point complex transform whose imaginary inputs are all zero.
template <typename T>
__global__ __launch_bounds__(FT, 8)        // (64 VGPRs: two workgroups of sixteen waves per CU -- at 69 only one fits, 1.15 -> 1.6 ms)
void tspec_kernel(TspecArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const sushi_fft::Twiddles tw = sushi_fft::load_twiddles<FFT_LOGN, -1>(tid, twiddles());
    const TspecSeg g = tspec_segment<FT>(a, tid);
    const T* __restrict__ t = (const T*)a.src_raw + g.off;
    const int len = g.len;
    const float t_sub = g.t_sub;
    cpx v[sushi_fft::PER];
#pragma unroll
    for (int r = 0; r < sushi_fft::PER; ++r) {
        const int e = sushi_fft::in_index<FFT_LOGN>(tid, r);
        const float xa = (float)t[e < len ? e : len - 1] - t_sub;
        v[r].x = e < len ? xa : 0.f;
        v[r].y = 0.f;
    }
    sushi_fft::fft_split<FFT_LOGN, -1>(v, tid, lds, tw);
    const float sc = g.sc;
    // The low entry straight to its place (sixteen half-written lines per wave, all completed by this workgroup within
    // microseconds) and the wave's share of the norm's SQUARE to the segment's accumulator (zeroed before the launch; slb_kernel
    // takes the root): staging both through the LDS, as spectra_kernel does once per stream, cost this kernel -- which runs every
    // step -- two barriers more and 0.6 ms of 1.0 at BASELINE configs[2].  Both leave BEFORE the hand-over: nothing of them stays live.
    {
        float rest2;
        const uint4 low = low_entry_and_rest(v, sc, tid, rest2);
        a.tspec_low[(size_t)blockIdx.x * LROWE + sushi_fft::lslot_of_thread(tid)] = low;
        const float w = wave_sum_shfl(rest2);
        if ((tid & 63) == 0) atomicAdd(a.tnorm_rest + blockIdx.x, w);
    }
    to_load_order(v, tid, lds);
    uint4* __restrict__ out = reinterpret_cast<uint4*>(a.tspec + (size_t)blockIdx.x * FN);
#pragma unroll
    for (int u = 0; u < sushi_fft::PER / 4; ++u)
        out[sushi_fft::wslot_uint4(tid, u)] = uint4{pack_h2(v[4 * u].x * sc, v[4 * u].y * sc), pack_h2(v[4 * u + 1].x * sc, v[4 * u + 1].y * sc),
                                                    pack_h2(v[4 * u + 2].x * sc, v[4 * u + 2].y * sc), pack_h2(v[4 * u + 3].x * sc, v[4 * u + 3].y * sc)};
}

// The real route (the default): the segment is real, so it is packed into HALF as many complex points, transformed by the
// 8192-point plan and unfolded (fft_core.hpp "Forward transform of a REAL, zero-padded pattern segment").  512 threads a segment,
// half the buffer: four workgroups of eight waves per CU, the complex route's residency.  The low rows and norms it leaves have the
// complex route's place and meaning.  A whole row's bins N - k are the conjugates of its bins k word for word, so it is stored as a
// HALF row (fft_core.hpp "HALF ROWS"): a thread's entries u = 0, 1 of its two rows -- thread 0: of row 0 and, as "row 1024", the
// conj-reversals of row 0's own mirrored entries.  The mirrors are still made in registers, for the low entries.
constexpr int RT = sushi_fft::RNT;
constexpr int RLDS_FLOATS = sushi_fft::lds_floats<sushi_fft::RLOGN>();
static_assert(2 * RT == FT && 2 * RLDS_FLOATS == LDS_FLOATS && sushi_fft::RN == FN && FFT_SEG * 4 == FN, "the real route's halves");
static_assert(HROWE == sushi_fft::HALF_ROWE && ROWE == 2 * sushi_fft::HALF_STORED, "sushi_geometry.hpp's half row is fft_core's");
template <typename T>
__global__ __launch_bounds__(RT, 8)        // (64 VGPRs, as the complex route)
void tspec_real_kernel(TspecArgs a) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    __shared__ __attribute__((aligned(16))) float lds[RLDS_FLOATS];
    const int tid = threadIdx.x;
    const sushi_fft::Twiddles tw = sushi_fft::load_twiddles<sushi_fft::RLOGN, -1>(tid, twiddles());
    const cpx wrow = twiddles()[sushi_fft::real_row(tid, 0)];
    const TspecSeg g = tspec_segment<RT>(a, tid);
    const T* __restrict__ t = (const T*)a.src_raw + g.off;
    const int len = g.len;
    const float t_sub = g.t_sub;
    cpx v[sushi_fft::PER];
#pragma unroll
    for (int r = 0; r < sushi_fft::PER; ++r) {
        // z[m] = x[2m] + i x[2m+1]; the registers whose samples lie past FFT_SEG (all but r = 0, 1, 8, 9: real_in_sample) are
        // zero as they stand
        const int e = sushi_fft::real_in_sample(tid, r);
        if ((r % sushi_fft::R1) < 2) {
            const float xa = (float)t[e < len ? e : len - 1] - t_sub;
            const float xb = (float)t[e + 1 < len ? e + 1 : len - 1] - t_sub;
            v[r].x = e < len ? xa : 0.f;
            v[r].y = e + 1 < len ? xb : 0.f;
        } else {
            v[r] = cpx{0.f, 0.f};
        }
    }
    sushi_fft::fft_split<sushi_fft::RLOGN, -1>(v, tid, lds, tw);
    // the hand-over: thread tid holds Z[tid + 512 r]; it takes the sixteen Z of its two rows, the tail's lanes their two of row 512 besides
    const bool tail = tid < sushi_fft::REAL_TAIL_LANES;
    cpx za[8], zb[8], tz = cpx{0.f, 0.f}, tp = cpx{0.f, 0.f}, tw_tail = cpx{0.f, 0.f};
    __syncthreads();                                             // the transform's own use of the buffer is over
    sushi_fft::real_z_store<0>(v, tid, lds);
    __syncthreads();
    sushi_fft::real_z_load<0>(za, zb, tid, lds);
    if (tail) {
        sushi_fft::real_tail_load<0>(tz, tp, tid, lds);
        tw_tail = twiddles()[sushi_fft::real_tail_z(tid, 0)];
    }
    __syncthreads();
    sushi_fft::real_z_store<1>(v, tid, lds);
    __syncthreads();
    sushi_fft::real_z_load<1>(za, zb, tid, lds);
    const float sc = 0.5f * g.sc;                                // (the unfold leaves twice the bins)
    uint32_t* __restrict__ row_words = a.tspec + (size_t)blockIdx.x * (4 * HROWE);
    uint4* __restrict__ low = a.tspec_low + (size_t)blockIdx.x * LROWE;
    auto abs2 = [](const unsigned w, const float acc) {
        const h2 h = __builtin_bit_cast(h2, w);
        return __builtin_amdgcn_fdot2(h, h, acc, false);
    };
    // The norm's square outside the band (bins 2 .. 13 of a row; row 0's bin 14, 7N/8, is counted with them and zero in its low
    // entry: low_entry_and_rest): a mirror has its bin's modulus exactly, so a thread's share is twice its own bins 2 .. 7 of
    // both rows -- thread 0: of row 0, and bin N/2 once.
    float e = 0.f;
    if (tail) {                                                  // row 512: bins tid and 7 - tid, word by word (their mirrors 15 - tid, 8 + tid: the low entry's only)
        sushi_fft::real_tail_load<1>(tz, tp, tid, lds);
        cpx lo, hi;
        sushi_fft::real_tail_bfly(tz, tp, tw_tail, lo, hi);
        const unsigned wlo = pack_h2(__builtin_fmaf(lo.x, sc, 0.f), __builtin_fmaf(lo.y, sc, 0.f));
        const unsigned whi = pack_h2(__builtin_fmaf(hi.x, sc, 0.f), __builtin_fmaf(hi.y, sc, 0.f));
        row_words[sushi_fft::half_tail_word(tid)] = wlo;
        row_words[sushi_fft::half_tail_word(7 - tid)] = whi;
        uint32_t* __restrict__ lw = reinterpret_cast<uint32_t*>(low + sushi_fft::lslot_of_thread(sushi_fft::REAL_TAIL_ROW));
        if (tid < 2) { lw[tid] = wlo; lw[3 - tid] = sushi_fft::real_conj_word(wlo); }       // bins 0, 1, 14, 15: the band
        e = abs2(whi, tid < 2 ? 0.f : abs2(wlo, 0.f));
    }
    cpx xa[8], xb[8];
    sushi_fft::real_unfold(za, zb, tid, wrow, xa, xb);
    unsigned wa[8], wb[8], ma[8], mb[8];
#pragma unroll
    for (int d = 0; d < 8; ++d) {                                // (+ 0: a zero is stored as +0 whatever sign the arithmetic left it)
        wa[d] = pack_h2(__builtin_fmaf(xa[d].x, sc, 0.f), __builtin_fmaf(xa[d].y, sc, 0.f));
        wb[d] = pack_h2(__builtin_fmaf(xb[d].x, sc, 0.f), __builtin_fmaf(xb[d].y, sc, 0.f));
    }
    sushi_fft::real_mirror_words(wa, wb, tid, ma, mb);
    const int ra = sushi_fft::real_row(tid, 0), rb = sushi_fft::real_row(tid, 1);
    {
        float eb = 0.f;
#pragma unroll
        for (int d = 2; d < 8; ++d) { e = abs2(wa[d], e); eb = abs2(wb[d], eb); }
        e = 2.f * (e + (tid == 0 ? 0.f : eb));
        if (tid == 0) e = abs2(wb[7], e);
        // the low entries (bins 0, 1, 14, 15 of a row) straight to their places and the wave's share of the norm's square to the
        // segment's accumulator (zeroed before the launch), as the complex route does
        low[sushi_fft::lslot_of_thread(ra)] = uint4{wa[0], wa[1], tid == 0 ? 0u : ma[6], ma[7]};
        if (tid != 0) low[sushi_fft::lslot_of_thread(rb)] = uint4{wb[0], wb[1], mb[6], mb[7]};
        const float w = wave_sum_shfl(e);
        if ((tid & 63) == 0) atomicAdd(a.tnorm_rest + blockIdx.x, w);
    }
    uint4* __restrict__ out = reinterpret_cast<uint4*>(row_words);
    out[sushi_fft::half_entry(ra, 0)] = uint4{wa[0], wa[1], wa[2], wa[3]};
    out[sushi_fft::half_entry(ra, 1)] = uint4{wa[4], wa[5], wa[6], wa[7]};
    // (thread 0, rb = 1024: the conj-reversals of row 0's entries 3 and 2 as they were stored whole -- its OWN bins 1 .. 7 and bin N/2,
    // not the second computation of them that its wb holds)
    out[sushi_fft::half_entry(rb, 0)] = tid != 0 ? uint4{wb[0], wb[1], wb[2], wb[3]} : uint4{wa[1], wa[2], wa[3], wa[4]};
    out[sushi_fft::half_entry(rb, 1)] = tid != 0 ? uint4{wb[4], wb[5], wb[6], wb[7]} : uint4{wa[5], wa[6], wa[7], wb[7]};
}

// Half rows -> the whole rows they stand for, entry by entry through the readers' own function (for
// sushi_hip_batch_workspace_view: tests and tools read whole rows).
__global__ __launch_bounds__(256)
void tspec_expand_kernel(const uint4* __restrict__ half_rows, uint4* __restrict__ whole_rows, const long long n_entries) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_entries; i += (long long)gridDim.x * 256)
        whole_rows[i] = sushi_fft::half_fetch(half_rows + (size_t)(i / ROWE) * HROWE, (int)(i % ROWE));
}
