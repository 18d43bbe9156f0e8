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
    uint32_t* tspec;                  // [segments of the sub-batch][FN] packed halves
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

template <typename T>
__global__ __launch_bounds__(FT, 8)        // (64 VGPRs: two workgroups of sixteen waves per CU -- at 69 only one fits, 1.15 -> 1.6 ms)
void tspec_kernel(TspecArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const sushi_fft::Twiddles tw = sushi_fft::load_twiddles<FFT_LOGN, -1>(tid, twiddles());
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
    const float t_sub = cc ? (float)ts_all.tmean : 0.f;
    const float y_scale = y_scale_for(tn_spec, (M + FFT_SEG - 1) / FFT_SEG, a.dst_stats[0]);
    const float t_scale = t_scale_for(tn_spec);
    if (s == 0) {
        const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, M);
        int* __restrict__ pm = a.pairmap + first_pair_in_sub(a.sub_first_pair, sd);
        for (int i = tid; i < lay.n_pairs; i += FT) pm[i] = k;
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
    const T* __restrict__ t = (const T*)a.src_raw + sd.tmpl_off + (int64_t)s * FFT_SEG;
    const int len = min(FFT_SEG, M - s * FFT_SEG);
    cpx v[sushi_fft::PER];
#pragma unroll
    for (int r = 0; r < sushi_fft::PER; ++r) {
        const int e = sushi_fft::in_index<FFT_LOGN>(tid, r);
        const float xa = (float)t[e < len ? e : len - 1] - t_sub;
        v[r].x = e < len ? xa : 0.f;
        v[r].y = 0.f;
    }
    sushi_fft::fft_split<FFT_LOGN, -1>(v, tid, lds, tw);
    const float sc = t_scale / (float)FN;
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
