// sushi_amd/csrc/sushi_fft_bound.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// the pair exclusion: bound_kernel / bound_low_kernel, slb_kernel, pilot / survivor kernels, the second look, whole rows of listed pairs.

// ------------------------------------------------------------------------------------------
// Which block pairs need no inverse transform at all.
//
// A position can be the search's arg-min only if its score is not above U, the smallest (f32 score + bound) any pair of the
// search has reported.  bound_kernel gives every pair a LOWER bound of the exact scores of all its positions without scoring
// any of them:
//   * the cross term: after the three passes of the inverse transform that stay inside a wave (no LDS exchange, no barrier),
//     wave n1 holds A_n1[k2], the 1024-point transform of its decimated share of Y, and every output of the full transform is
//     a sum of sixteen of them times unit factors: |y[r]| <= B = sum_n1 max_k2 |A_n1[k2]|.  For a pair that does not hold the
//     match the A are noise and B is a fifth of what the matching pair's is;
//   * the window energies: sum I^2 over [p, p + M) >= S2[(j + M / G) G] - S2[(j + 1) G] for every p of the G-sample stretch j
//     (a table of the prefix at every G = COARSE_G-th sample, built once per stream); wlb = the smallest over the pair's
//     stretches that hold a valid position;
//   * score(p) = (sum T^2 + wU - 2 sum T I) / (|T| sqrt(wU)) increases with wU and decreases with sum T I, so
//         slb = (tU' + wlb - 2 Ymax) / (|T| sqrt(wlb)),   Ymax = B / scale + the cross term's modelled error (pair_error_model)
//     is below every exact score of the pair.
// pilot_kernel then picks, per search, the pair with the smallest slb -- where the match is if there is one --, ifft_kernel
// transforms and scores those (one workgroup per search) and leaves U; survivor_kernel lists the pairs with slb <= U, which are
// transformed as before; all others are done: slb > U means every exact score of the pair is above the exact score of a position
// already found.  (U >= 1 -- nothing matches anywhere, every score clamps to 1 and TIES -- excludes nothing.)
// ------------------------------------------------------------------------------------------
struct BoundArgs {
    const uint2* y;
    const double* dst_stats;
    const SearchDesc* searches;       // the sub-batch's searches
    int sub_first_pair;
    int first_search;
    int64_t dst_len;
    const int* pairmap;
    const TemplConsts* tconst;
    const double* ubase;
    const double* sbase;
    int64_t nb;
    const double* coarse;             // [nc] s2 at every COARSE_G-th sample
    int64_t nc;
    float* slb;                       // [pairs of the sub-batch] out: lower bound of the pair's exact scores (-inf: none)
    float* acc;                       // [pairs of the sub-batch][2] bound_kernel's accumulators: sum of the waves' max |A|, largest wave row energy
    // pilot / survivor stages
    int n_sub;
    int n_pairs;
    int* plist;                       // [searches of the sub-batch] the pair transformed first
    int* slist;                       // [pairs of the sub-batch] the pairs still to transform
    int* scount;                      // [1]
    const int* order;                 // the L2-friendly schedule of all pairs (survivors keep its order)
    const unsigned long long* gkeys;  // [all searches]
    float* pair_lb;
    RunCounters* counters;
    // band-split form (bound_low_kernel: `y` = the low rows; slb_kernel adds the rest of the spectrum from the rows' norms)
    int band;                         // 0: `acc` is over whole rows (bound_kernel); 1: over low rows + norms; 2: norms only (prediction)
    int sub_first_seg;
    const float* tnorm_rest;          // [segments of the sub-batch] pattern spectra: SQUARED norm outside the band
    const float* znorm_rest;          // [3][norm_stride] block spectra: norm outside the band of Z, of its real block at j B, of the one H on
    int64_t norm_stride;
    int* band_votes;                  // [VOTE_SLOTS][VOTE_STRIDE] prediction: per slot [0] pairs looked at, [1] pairs whose bound leaves room
    unsigned char* audit_mark;        // [pairs of the sub-batch] MARK_* bits (sushi_internal.hpp): MARK_AUDITED, MARK_LISTED, MARK_SECOND_LOOK
    unsigned audit_seq;               // changes from run to run: which excluded pair of a search is audited
    int audit_every;                  // one search in this many is audited per run (0: none)
    int worst_case;                   // 1: every rounding on the excluded side enters at its WORST CASE (slb_one; the default); 0: round 5's statistical model
    float half_err;                   // what a packed-half transform output may be off by, in units of the largest pass-1 value (bound_low_kernel / bound_kernel)
    const int* list;                  // slb_list_kernel / bound_low_exact_kernel / survivor2_kernel: the pairs the first bound left ...
    const int* list_count;            // ... how many
    int* list2;                       // survivor2_kernel: the pairs the second look left ...
    int* list2_count;                 // ... how many
};

// Stage 1 of the band-split form.  A wave takes a PAIR: the eight groups of its low row one after the other (2 KB each, the next
// one requested before the current one is transformed), each through the three in-wave passes of its half-empty 1024-point
// transform in packed halves (fft_core.hpp "LOW BAND").  Every lane register holds the same output index k for every group, so
// the sum over the groups stays in registers: with y_low[2 r'] = sum_g w^(g r') A_g[r' mod 1024],
//     |y_low[2 r']| <= sum_g |A_g[k]| <= sqrt(8 sum_g |A_g[k]|^2)             (Cauchy-Schwarz over the eight groups)
// -- one v_dot2 per value, no square root, no exchange between waves -- and the largest of that over k bounds the low band's
// transform at its sample points (the sum of the groups' separate maxima is 1.7 x looser).  The halves' rounding (header of the
// packed-half passes: every |A_g| may be 0.2 % + 0.29 x the largest pass-1 value off) goes on top by Minkowski's inequality.
// Persistent, free-running waves; acc[2 pr] = the bound, acc[2 pr + 1] = the low row's energy (plain stores: one wave per pair).
// NEED_Q: also the low row's energy (acc[2 pr + 1]), which only the STATISTICAL model of the roundings reads (slb_one) -- the worst
// case, the default, does not: sixteen dot products and a wave reduction per group less.
template <bool NEED_Q>
__global__ __launch_bounds__(256, 3)
void bound_low_kernel(BoundArgs a) {
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * 4;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t n_items = (int64_t)a.n_pairs * sushi_fft::LB_GROUPS;
    const sushi_fft::MfmaBl mb = sushi_fft::load_mfma_bl(lane, reinterpret_cast<const sushi_fft::uint2v*>(g_dft16_bl));
    const sushi_fft::HTwiddles tw = sushi_fft::load_htwiddles(lane, twiddles());
    const sushi_fft::uint4v* __restrict__ yh = reinterpret_cast<const sushi_fft::uint4v*>(a.y);
    auto load_item = [&](const int64_t it, sushi_fft::uint4v (&yl)[4]) {
        // item = pair * 8 + group: a pair's groups are consecutive 2 KB pieces of its row (the upper lanes re-read the lower lanes' entries)
#pragma unroll
        for (int u = 0; u < 4; ++u) yl[u] = yh[(size_t)it * (LROWE / sushi_fft::LB_GROUPS) + u * 32 + (lane & 31)];
    };
    if (gw >= a.n_pairs) return;
    sushi_fft::uint4v yl[4], yn[4];
    load_item((int64_t)gw * sushi_fft::LB_GROUPS, yl);
    for (int64_t pr = gw; pr < a.n_pairs; pr += waves) {
        float msum[sushi_fft::PER];
#pragma unroll
        for (int r = 0; r < sushi_fft::PER; ++r) msum[r] = 0.f;
        float q2 = 0.f, d2 = 0.f, dc_re = 0.f, dc_im = 0.f;
        for (int g = 0; g < sushi_fft::LB_GROUPS; ++g) {
            // the next group of this pair, or the first of the wave's next pair (the very last one re-requests itself)
            int64_t nx = pr * sushi_fft::LB_GROUPS + g + 1;
            if (g == sushi_fft::LB_GROUPS - 1) nx = pr + waves < a.n_pairs ? (pr + waves) * sushi_fft::LB_GROUPS : nx - 1;
            nx = nx < n_items ? nx : n_items - 1;
            load_item(nx, yn);
            __builtin_amdgcn_sched_barrier(0);
            typedef _Float16 h2 __attribute__((ext_vector_type(2)));
            if (NEED_Q) {
                float q = 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) q = add_abs2_entry(yl[u], q);
                q2 += lane < 32 ? q : 0.f;
            }
            if (g == 0) {
                // Bin 0 apart: a pattern that is not centred (TM_SQDIFF_NORMED) meets whatever a stretch of the stream sums to
                // beside the stream's mean -- a constant under every output of the pair, often the largest single bin, and
                // with it in, one of the eight groups dwarfs the others (the Cauchy-Schwarz step above is then 2.8 x loose).
                // It is entry 0, sub-position 0 of the row (lb_bin_of); its real / imaginary part is added back SIGNED below.
                const h2 y0 = __builtin_bit_cast(h2, (unsigned)__builtin_amdgcn_readfirstlane((int)yl[0][0]));
                dc_re = (float)y0.x; dc_im = (float)y0.y;
                if ((lane & 31) == 0) yl[0][0] = 0u;
            }
            sushi_fft::h2 v[sushi_fft::PER];
            unsigned in2;
            sushi_fft::fft_wave_half_front_low(yl, v, tw, mb, in2);
            d2 += a.half_err * a.half_err * __uint_as_float(wave_max_u32(in2));   // (half_err x this group's largest pass-1 value)^2
#pragma unroll
            for (int r = 0; r < sushi_fft::PER; ++r) msum[r] = __builtin_amdgcn_fdot2(v[r], v[r], msum[r], false);
#pragma unroll
            for (int u = 0; u < 4; ++u) yl[u] = yn[u];
        }
        unsigned m2 = 0u;
#pragma unroll
        for (int r = 0; r < sushi_fft::PER; ++r) m2 = sushi_fft::h_max_bits(m2, __float_as_uint(msum[r]));   // (sums of squares: >= 0)
        const unsigned wm = wave_max_u32(m2);
        const float qw = NEED_Q ? wave_sum_f32(q2) : 0.f;
        if (lane == 0) {
            // sqrt(8) (sqrt(max_k sum_g |A_g[k]|^2) (1 + 0.2 %) + sqrt(sum_g (0.29 max |pass-1 value of g|)^2)), the 2^-10 undone:
            // the modulus of the band (bin 0 aside) at its sample points; sqrt(2) more everywhere between them (fft_core.hpp
            // "LOW BAND"); plus bin 0's own part, signed -- the cross term's real parts score the pair's first half, its imaginary
            // parts the second: an UPPER bound of both is what a lower bound of the scores needs
            float bw = 1.4142137f * 2.8284272f * (sqrtf(__uint_as_float(wm)) * 1.002f + sqrtf(d2)) * 1024.0f + fmaxf(dc_re, dc_im);
            if (wm >= 0x7f800000u || !(d2 < __builtin_inff())) bw = __builtin_inff();
            a.acc[2 * (size_t)pr] = bw;
            a.acc[2 * (size_t)pr + 1] = qw * 1.000001f;
        }
    }
}

// Stage 1: the transform part.  An item = (pair, n1): one wave's decimated share of one pair's Y (4 KB), three passes, the
// largest |A_n1[k2]|.  Waves are persistent and free-running -- no workgroup-wide step: every wave walks its own items and
// requests the next item's Y before it transforms the current one, so that the HBM stream never waits for a transform (with
// one workgroup per pair, all sixteen waves loading and then all sixteen transforming, it ran at half the rate).  Neighbouring
// waves take neighbouring items: the sixteen shares of a pair are read at about the same time.  Results are added to the pair's
// accumulators (zeroed by a memset): acc[2 pr] += max |A|, acc[2 pr + 1] = max(row energy of a wave) as float bits.
constexpr int BOUND_THREADS = 256;
template <bool NEED_Q>          // (bound_low_kernel: the row energy is the statistical model's only)
__global__ __launch_bounds__(BOUND_THREADS, 4)
void bound_kernel(BoundArgs a) {
    const int lane = threadIdx.x & 63;
    const int waves = gridDim.x * (BOUND_THREADS / 64);
    const int gw = blockIdx.x * (BOUND_THREADS / 64) + (threadIdx.x >> 6);
    const int64_t n_items = (int64_t)a.n_pairs * 16;
    // the transform's per-lane constants do not depend on the wave: loaded (and rounded to halves) once
    const sushi_fft::MfmaBh mb = sushi_fft::load_mfma_bh(lane, reinterpret_cast<const sushi_fft::uint4v*>(g_dft16_bh));
    const sushi_fft::HTwiddles tw = sushi_fft::load_htwiddles(lane, twiddles());
    const sushi_fft::uint4v* __restrict__ yh = reinterpret_cast<const sushi_fft::uint4v*>(a.y);
    auto load_item = [&](const int64_t it, sushi_fft::uint4v (&yl)[4]) {
        const size_t pr = (size_t)(it >> 4);
        const int n1 = (int)(it & 15);
#pragma unroll
        for (int u = 0; u < 4; ++u) yl[u] = yh[pr * (FN / 4) + sushi_fft::wslot_uint4(n1 * 64 + lane, u)];
    };
    int64_t it = gw;
    if (it >= n_items) return;
    sushi_fft::uint4v yl[4], yn[4];
    load_item(it, yl);
    for (; it < n_items; it += waves) {
        const int64_t nx = it + waves < n_items ? it + waves : it;       // (the last item re-requests itself: unconditional loads)
        load_item(nx, yn);
        __builtin_amdgcn_sched_barrier(0);      // (left to itself the scheduler sinks these loads to the end of the loop body: no prefetch at all)
        float q2 = 0.f;
        if (NEED_Q) {
#pragma unroll
            for (int u = 0; u < 4; ++u) q2 = add_abs2_entry(yl[u], q2);
        }
        // the three in-wave passes in packed halves (fft_core.hpp): 2^-10 A_n1[k2], good to two digits -- enough for a bound
        sushi_fft::h2 v[sushi_fft::PER];
        unsigned in2;
        sushi_fft::fft_wave_half_front(yl, v, tw, mb, in2);
        unsigned m2 = 0u;                                                  // largest |value|^2 as float bits (fft_core.hpp h_abs2)
#pragma unroll
        for (int r = 0; r < sushi_fft::PER; ++r) m2 = sushi_fft::h_max_bits(m2, sushi_fft::h_abs2(v[r]));
        const unsigned wm = wave_max_u32(m2), wi = wave_max_u32(in2);
        const float qw = NEED_Q ? wave_sum_f32(q2) : 0.f;
        if (lane == 0) {
            const size_t pr = (size_t)(it >> 4);
            // the largest |A|: what the halves gave, their rounding (header of the packed-half passes), the 2^-10 undone
            float bw = (sqrtf(__uint_as_float(wm)) * 1.002f + a.half_err * sqrtf(__uint_as_float(wi))) * 1024.0f;
            if (wm >= 0x7f800000u || wi >= 0x7f800000u) bw = __builtin_inff();
            atomicAdd(a.acc + 2 * pr, bw);
            if (NEED_Q) atomicMax(reinterpret_cast<unsigned*>(a.acc + 2 * pr + 1), __float_as_uint(qw));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) yl[u] = yn[u];
    }
}

// Stage 2: one wave per pair puts the bound together (header above): B and the row energy from the accumulators, the lower
// bound of the window energies from the coarse table, the FFT stage's error from the block bases.
// TM_CCOEFF_NORMED (ranked as 1 - cc): cc(p) = sum (T - mean T) I / (|T_c| sqrt(d2(p))) <= Ymax / (|T_c| sqrt(d2lb)) with
//   d2(p) = sum over the window of (I - c)^2  -  (sum over the window of (I - c))^2 / M          (a variance sum: any c)
//         >= Ein(j) - (|Din(j)| + sqrt(2 G (Eout(j) - Ein(j))))^2 / M
// for every p of stretch j: Ein / Din = energy / sum of the centred samples over the G-aligned span inside every such window,
// Eout = the energy over the G-aligned span around every such window; what a window holds beyond the inner span is at most 2 G
// samples of at most Eout - Ein energy (Cauchy-Schwarz).  A flat window anywhere in the pair makes d2lb <= 0: nothing excluded.
//
// GROUP lanes take a pair (`lane`: the lane inside its group; `live`: the group has a pair -- an idle one is given another
// group's, loads like it and stores nothing).  GROUP = 64 is the wave a pair (slb_one: pair, search and constants wave-uniform).
// GROUP = SLB_GROUP = 16, four pairs a wave (slb_four), for patterns of up to 16 segments: a lane looks up six stretches instead
// of two, still in one flight; the window energies' minimum and the norm sums are taken inside the group's row of sixteen lanes
// -- a minimum does not depend on the order, and the sums are row_reduce_f32's, what wave_reduce_f32 starts with: the whole wave's
// sum is the first row's plus exact zeros --; and the epilogue, ~300 wave-instructions of float64 on one lane, is issued once for
// the four pairs, on the first lane of every group.  Every stored value has the bits the wave a pair gives it.
constexpr int SLB_GROUP = 16;
template <int METHOD, int GROUP>
__device__ __forceinline__ void slb_body(const BoundArgs& a, const int pr, const int lane, const bool live, const int k, const SearchDesc sd) {
    constexpr bool CC = METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    static_assert(GROUP == 64 || GROUP == SLB_GROUP, "a wave or a row of sixteen lanes");
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const int64_t pairI = absolute_pair(lay, a.sub_first_pair, pr, sd);
    const int64_t qbase = pairI * FFT_STEP * (int64_t)FFT_SEG;
    const int M = sd.tmpl_len;
    const TemplConsts tc = a.tconst[k];
    const int64_t kA = pairI * FFT_STEP;
    const int n_seg = lay.n_seg;
    const int64_t n = a.dst_len;
    const double c = a.dst_stats[1];
    // A wave is a chain of dependent look-ups (pair -> search -> constants -> tables), 354,555 of them at BASELINE configs[2]: what
    // it costs is round trips, not instructions.  So EVERYTHING the wave will read is requested here in one flight, raw, and used
    // only after the table look-ups have been requested too.
    const float acc0 = a.acc[2 * (size_t)pr], acc1 = a.acc[2 * (size_t)pr + 1];
    const int64_t iA = kA < a.nb ? kA : a.nb, iB = kA + n_seg + 2 * FFT_VB < a.nb ? kA + n_seg + 2 * FFT_VB : a.nb;
    const double u0 = a.ubase[iA], u1 = a.ubase[iB], s0 = a.sbase[iA], s1 = a.sbase[iB];
    // band-split form: what the bins outside the band can add to any output of the pair's transform, from the norms of the rows
    // that meet (Cauchy-Schwarz per segment, the triangle inequality over the segments; the stored halves' own rounding and
    // their subnormal floor on top; a pattern of more than MAC_SMAX_LONG segments re-rounds its partial row once per pass).
    // The real parts of the pair's outputs meet the real blocks at 6 I + s, the imaginary parts those H samples on: each from
    // its own block's norm (real_block_rest_norms) -- the larger of the two sums bounds both parts.  That split assumes the
    // pattern rows conjugate-symmetric (spectra of real segments); what their stored halves lack of it (half an ulp per bin
    // and the float32 transform's own asymmetry: < 1.5e-3 of a row's norm) meets the whole |Z|.
    // (unconditional loads from clamped places -- a branch around them would be a second flight --, masked afterwards)
    const int sl = lane < n_seg ? lane : 0;
    const int64_t jl = kA + sl < a.nb ? kA + sl : a.nb;
    float tn0 = a.tnorm_rest[(sd.first_seg - a.sub_first_seg) + sl];
    const float zn0 = a.znorm_rest[jl], an0 = a.znorm_rest[a.norm_stride + jl], bn0 = a.znorm_rest[2 * a.norm_stride + jl];
    // lower bound of the window energies (variance sums): the stretches of COARSE_G positions that hold a valid position
    constexpr int NSB = 2 * FH / COARSE_G;
    static_assert(NSB <= 128 && (FFT_STEP * FFT_SEG) % COARSE_G == 0, "a lane looks up two stretches");
    constexpr int NSL = slb_stretches_a_lane(GROUP);            // stretches a lane looks up: two of a wave's, six of a group's
    static_assert(NSL * GROUP >= NSB && (GROUP == 64 ? NSL == 2 : NSL * GROUP == NSB), "the group's lanes cover the stretches");
    const int64_t plo = sd.win_start - qbase, phi = (int64_t)sd.n_pos + (sd.win_start - qbase);       // valid: plo <= pos < phi
    const double* __restrict__ c2 = a.coarse;
    const double* __restrict__ c1 = a.coarse + a.nc;
    auto clampi = [&](int64_t x) { return x < a.nc - 1 ? x : a.nc - 1; };
    // (every stretch of a lane: unconditional loads from clamped places, the stretch's validity applied afterwards)
    bool use[NSL];
    int64_t js[NSL], je[NSL], jo0[NSL], jo1[NSL];
    double c2e[NSL], c2s[NSL], c1e[NSL], c1s[NSL], c2o1[NSL], c2o0[NSL], c1o1[NSL], c1o0[NSL];
#pragma unroll
    for (int t = 0; t < NSL; ++t) {
        const int sb = slb_stretch(lane, t, GROUP);
        const int64_t p0 = (int64_t)sb * COARSE_G;
        use[t] = sb < NSB && p0 + COARSE_G > plo && p0 < phi;
        const int64_t j = qbase / COARSE_G + sb;
        js[t] = clampi(j + 1); je[t] = clampi(j + M / COARSE_G);
        c2e[t] = c2[je[t]]; c2s[t] = c2[js[t]];
        if (CC) {
            jo0[t] = clampi(j); jo1[t] = clampi(j + M / COARSE_G + 2);
            c1e[t] = c1[je[t]]; c1s[t] = c1[js[t]];
            c2o1[t] = c2[jo1[t]]; c2o0[t] = c2[jo0[t]]; c1o1[t] = c1[jo1[t]]; c1o0[t] = c1[jo0[t]];
        }
    }
    __builtin_amdgcn_sched_barrier(0);          // (nothing that uses a loaded value moves above this line: one flight)
    float wl = __builtin_inff();
#pragma unroll
    for (int t = 0; t < NSL; ++t) {
        if (use[t]) {
            double e = 0.0;
            if (je[t] > js[t]) {
                if (CC) {
                    auto len = [&](int64_t lo, int64_t hi) {
                        const int64_t x0 = lo * COARSE_G < n ? lo * COARSE_G : n, x1 = hi * COARSE_G < n ? hi * COARSE_G : n;
                        return (double)(x1 - x0);
                    };
                    const double d_in = (c1e[t] - c1s[t]) - c * len(js[t], je[t]);
                    const double e_in = (c2e[t] - c2s[t]) - 2.0 * c * (c1e[t] - c1s[t]) + c * c * len(js[t], je[t]);
                    const double e_out = (c2o1[t] - c2o0[t]) - 2.0 * c * (c1o1[t] - c1o0[t]) + c * c * len(jo0[t], jo1[t]);
                    const double d_ub = fabs(d_in) + sqrt(2.0 * COARSE_G * fmax(e_out - e_in, 0.0)) * 1.000001 + 1e-6 * (fabs(d_in) + 1.0);
                    e = e_in * 0.999999 - d_ub * d_ub / (double)M - 1e-9 * (c2e[t] - c2s[t]);    // (the prefix table's own rounding)
                } else {
                    e = c2e[t] - c2s[t];
                }
            }
            wl = fminf(wl, fmaxf((float)e * 0.9999995f, 0.f));
        }
    }
    auto group_min = [](float v) {
        if constexpr (GROUP == 64) return wave_min_f32(v);
        else return row_reduce_f32(v, [](float x, float y) { return fminf(x, y); });
    };
    auto group_sum = [](float v) {
        if constexpr (GROUP == 64) return wave_sum_f32(v);
        else return row_reduce_f32(v, [](float x, float y) { return x + y; });
    };
    const float wlb = group_min(wl);
    float b_rest = 0.f;
    if (a.band) {
        const float t0n = lane < n_seg ? sqrtf(tn0) * 1.000002f : 0.f;
        float pz = t0n * zn0, pa = t0n * an0, pb = t0n * bn0;
        // (a group's products go into its reduction as ROUNDED products, as the wave's do, whose loop below carries them: left to
        // itself the compiler contracts each into the reduction's first addition, and a sum's last bit changes now and then)
        if constexpr (GROUP != 64) asm volatile("" : "+v"(pz), "+v"(pa), "+v"(pb));
        if constexpr (GROUP == 64) {
            for (int s = lane + 64; s < n_seg; s += 64) {               // (patterns of more than 64 segments)
                const int64_t jj = kA + s < a.nb ? kA + s : a.nb;
                const float t = sqrtf(a.tnorm_rest[(sd.first_seg - a.sub_first_seg) + s]) * 1.000002f;
                pz += t * a.znorm_rest[jj]; pa += t * a.znorm_rest[a.norm_stride + jj]; pb += t * a.znorm_rest[2 * a.norm_stride + jj];
            }
        }
        pz = group_sum(pz); pa = group_sum(pa); pb = group_sum(pb);
        const int passes = (n_seg + MAC_SMAX_LONG - 1) / MAC_SMAX_LONG;
        b_rest = (fmaxf(pa, pb) + 1.5e-3f * pz) * tc.mac_scale * (1.0006f + 0.0005f * (float)passes) + 1e-3f;
    }
    if (lane == 0 && live) {
        float B = acc0, qmax = acc1;
        if (a.band) {
            // acc[1] is the low band's energy, and the rest's is at most the square of its sum of moduli -- as one sixteenth of a
            // row's energy, the unit the model below takes
            B = (a.band == 2 ? 0.f : B) + b_rest;                 // (bound_low_kernel's value is complete: sqrt(2) and bin 0 are in it)
            qmax = ((a.band == 2 ? 0.f : qmax) + b_rest * b_rest) * (1.0f / (float)(FT / 64));
        }
        // energy of the samples that enter this pair's transforms, as they are (zn) and centred (zn_c): score_pair's
        const int64_t s_lo = qbase < n ? qbase : n;
        const int64_t s_hi64 = (kA + n_seg + 2 * FFT_VB) * (int64_t)FFT_SEG;
        const int64_t s_hi = s_hi64 < n ? s_hi64 : n;
        const double e2 = (u1 - u0) - 2.0 * c * (s1 - s0) + c * c * (double)(s_hi - s_lo);
        const double zn_c = sqrt(fmax(e2, 0.0)) * 1.0000005, zn = sqrt(fmax(u1 - u0, 0.0)) * 1.0000005;
        const int mac_passes = (n_seg + MAC_SMAX_LONG - 1) / MAC_SMAX_LONG;
        const double sigma_y = sqrt((double)((float)(FT / 64) * qmax) * (7.9472862e-8 * (double)(2 + mac_passes)) + (double)FN * 1.2e-15) *
                               (double)tc.inv_scale;
        // what the exact cross term of any position of this pair can reach: the bound of the transform's outputs (its own
        // float32 rounding included in the factor), the FFT stage's error, the packed halves' modelled error
        const double tn = CC ? (tc.inv_tnorm_c > 0.f ? 1.0 / (double)tc.inv_tnorm_c : 0.0) : (double)tc.tnorm;
        // (an UPPER bound of the signed cross term: the band-split form's may be negative)
        double ymax = (double)B * (double)tc.inv_scale + fabs((double)B) * (double)tc.inv_scale * 2e-5;
        if (a.worst_case) {
            // THE EXCLUDED SIDE IS A PROOF, NOT A MODEL (VERDICT r5 item 1).  B bounds the transform of the halves AS STORED; the exact
            // cross term differs from that by what the stored halves differ from the exact spectra by, every term at its worst case
            // with all of them in phase (triangle inequality over the bins, no independence assumed):
            //   |y[r] - y_stored[r]| <= sum_f |Tt Z - stored product|(f)
            //      <= (2 u_h + 2 e_F + g) sum_s sum_f |Tt_s(f)| |Z_s(f)|  +  (passes) u_h sum_f |Y(f)|       u_h = 2^-11: a half's rounding
            //      <= c sum_s |Tt_s| |Z_s|   (Cauchy-Schwarz over ALL bins, band and rest alike)
            //      =  c sum_s |t_s| |z_s|    (Parseval: segment s of the pattern, the 2 N centred samples block 6 I + s packs)
            //      <= c |T| sqrt(sum_s |z_s|^2) <= c |T| sqrt(8) zn_c
            // (every sample of the pair's span of n_seg + 6 blocks enters at most four block spectra as a first and four as a second
            // half).  e_F = 1e-5 >= 14 (mu + g_4 (sqrt 2 + mu)): the float32 forward transforms' relative error in the 2-norm (Higham,
            // Accuracy and Stability of Numerical Algorithms, Thm 24.2, log2 N = 14 radix-2 levels, twiddles good to 4 u: 8.06e-6;
            // the pattern rows' real-input route is 13 such levels, one rounded addition and one more such level -- its unfold --:
            // 14 (...) + u = 8.12e-6, DESIGN.md 3.3);
            // g <= 2e-5: mac_kernel's float32 sums.  The same terms cover what the NORMS of the stored rows outside the band differ
            // from the exact rows' by, and what the stored pattern rows lack of conjugate symmetry.  The halves' subnormal floor
            // (2^-25 absolute per stored value, N bins a row): of the pattern rows < 1.3e-9 sqrt(n_seg) |T| zn_c (inside c), of the block
            // rows 3.3e-10 sqrt(n_seg) |T| sqrt(E7) (1 / the stream's scale <= 0.01105 sqrt(E7)), of Y itself N 2^-25 of its units.
            const double c_wc = (double)(mac_passes + 2) * 4.8829e-4 * 1.001 + 4e-5;
            const double zn_wc = CC ? fmax(zn, zn_c) : zn_c;
            ymax += c_wc * 2.8284272 * tn * zn_wc
                  + 3.3e-10 * sqrt((double)n_seg) * tn * sqrt(fmax(a.dst_stats[0], 0.0)) + 5e-4 * (double)tc.inv_scale;
        } else {
            ymax += 5.9604645e-8 * (double)FFT_KE * (CC ? fmax(zn, zn_c) : zn_c) * tn + (double)Y_KQ * sigma_y;
        }
        float slb = -__builtin_inff();
        bool room = false;          // (prediction) the bound, with nothing but the norms outside the band in it, keeps 55 % of what a zero cross term would score
        if (CC) {
            if (wlb > 0.f && wlb < __builtin_inff() && !tc.flat && tn > 0.0) {
                slb = (float)(1.0 - ymax / (tn * sqrt((double)wlb)) * 1.000001);
                room = slb > 0.55f;
            }
        } else {
            const double t0 = tc.tU - 2.0 * (double)tc.c_sum_t;
            const double a0 = t0 - 2.0 * ymax;
            if (wlb > 0.f && wlb < __builtin_inff() && a0 < (double)wlb && tc.tU > 0.0) {
                slb = (float)((a0 + (double)wlb) / (sqrt((double)wlb) * (double)tc.tnorm) * 0.999999);
                room = a0 + (double)wlb >= 0.55 * (t0 + (double)wlb);
            }
        }
        a.slb[pr] = slb;
        if (a.band == 2) {
            // prediction: with NOTHING from the low band, does the rest alone leave the bound room to exclude?  (The scores'
            // scale is what a zero cross term gives -- small for streams that sit on a large mean --: the rest may take 45 % of it,
            // the low band's sum and the match's own score need the other half.)
            // (one of VOTE_SLOTS counters a cache line apart, by the pair's index: every pair adding to the same two words took 9 ms
            // at BASELINE configs[2] -- same-address atomics serialise in the L2 --, all of it in front of the batch's first run)
            int* __restrict__ v = a.band_votes + (size_t)(pr & (VOTE_SLOTS - 1)) * VOTE_STRIDE;
            atomicAdd(v, 1);
            if (room) atomicAdd(v + 1, 1);
        }
    }
}
// a wave a pair
template <int METHOD>
__device__ __forceinline__ void slb_one(const BoundArgs& a, const int pr, const int lane) {
    const int k = __builtin_amdgcn_readfirstlane(a.pairmap[pr]);
    const SearchDesc sd = a.searches[k];
    slb_body<METHOD, 64>(a, pr, lane, true, k, sd);
}
// A wave takes the four pairs at `first` .. `first` + 3 of `count` (`pair_at`: entry -> pair; `first` < `count`), a group of
// sixteen lanes each; a tail's idle groups are given the first pair.  Where one of the four has a pattern of more than SLB_GROUP
// segments -- its norms would not fit a row of lanes --, the four are taken one after the other, a wave a pair.
template <int METHOD, class PairAt>
__device__ __forceinline__ void slb_four(const BoundArgs& a, const int first, const int count, const PairAt pair_at, const int lane) {
    const int entry = first + lane / SLB_GROUP;
    const bool live = entry < count;
    const int pr = pair_at(live ? entry : first);
    const int k = a.pairmap[pr];
    const SearchDesc sd = a.searches[k];
    if (__all(fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len).n_seg <= SLB_GROUP)) {
        slb_body<METHOD, SLB_GROUP>(a, pr, lane % SLB_GROUP, live, k, sd);
        return;
    }
    for (int e = first; e < first + 64 / SLB_GROUP && e < count; ++e)
        slb_one<METHOD>(a, __builtin_amdgcn_readfirstlane(pair_at(e)), lane);
}
template <int METHOD>
__global__ __launch_bounds__(256)
void slb_kernel(BoundArgs a) {
    const int first = __builtin_amdgcn_readfirstlane((blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / SLB_GROUP));
    if (first >= a.n_pairs) return;
    slb_four<METHOD>(a, first, a.n_pairs, [](const int e) { return e; }, threadIdx.x & 63);
}
// the same for the pairs of a list (the second look at what the first bound left: bound_low_exact_kernel)
template <int METHOD>
__global__ __launch_bounds__(256)
void slb_list_kernel(BoundArgs a) {
    const int n = *a.list_count;
    if (n > a.n_pairs / 5) return;                      // (nothing was excluded to speak of: no second look either)
    const int step = gridDim.x * 4 * (64 / SLB_GROUP);
    for (int first = (blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 / SLB_GROUP); first < n; first += step)
        slb_four<METHOD>(a, first, n, [&](const int e) { return a.list[e]; }, threadIdx.x & 63);
}
// a wave a pair throughout (SUSHI_HIP_SLB=wave: the kernels before the groups, for A/B runs on one build)
template <int METHOD>
__global__ __launch_bounds__(256)
void slb_wave_kernel(BoundArgs a) {
    const int pr = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (pr >= a.n_pairs) return;
    slb_one<METHOD>(a, pr, threadIdx.x & 63);
}
template <int METHOD>
__global__ __launch_bounds__(256)
void slb_list_wave_kernel(BoundArgs a) {
    const int n = *a.list_count;
    if (n > a.n_pairs / 5) return;
    const int waves = gridDim.x * 4;
    for (int slot = blockIdx.x * 4 + (threadIdx.x >> 6); slot < n; slot += waves)
        slb_one<METHOD>(a, __builtin_amdgcn_readfirstlane(a.list[slot]), threadIdx.x & 63);
}

// THE TESTS' SEAM (SUSHI_HIP_TEST_BOUND_FAULT=<period>:<phase>[:<pair>], DESIGN.md 3.2; sushi_hip_batch_create parses it): the
// bounds of chosen pairs made WRONG on purpose, so that the suite can see the audit catch a wrong bound and every run kind
// recover from it.  The stored bound of every pair (`pair` < 0) or of the pair with index `pair` inside its search, of every
// search whose batch-wide index g has g % period == phase, becomes +inf: "no score of this pair can be any good".  A kernel
// of its own, launched behind slb_kernel and slb_list_kernel only by a batch that carries a fault (period > 0): without the
// variable no launch, no argument and no kernel differs.
struct BoundFaultArgs {
    const SearchDesc* searches;       // the sub-batch's searches
    const int* pairmap;
    float* slb;
    int first_search, sub_first_pair, n_pairs;
    BoundFault f;
};
__global__ __launch_bounds__(256)
void bound_fault_kernel(BoundFaultArgs a) {
    const int pr = blockIdx.x * 256 + threadIdx.x;
    if (pr >= a.n_pairs) return;
    const int k = a.pairmap[pr];
    if ((unsigned)(a.first_search + k) % (unsigned)a.f.period != (unsigned)a.f.phase) return;
    if (a.f.pair >= 0 && pair_of_search(a.sub_first_pair, pr, a.searches[k]) != a.f.pair) return;
    a.slb[pr] = __builtin_inff();
}

// per search: the pair with the smallest lower bound (the first of them) is transformed first
__global__ __launch_bounds__(64)
void pilot_kernel(BoundArgs a) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const SearchDesc sd = a.searches[k];
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const int p0 = first_pair_in_sub(a.sub_first_pair, sd);
    unsigned long long best = NO_KEY;
    for (int i = lane; i < lay.n_pairs; i += 64) {
        const float s = a.slb[p0 + i];
        // order-preserving key of a float that may be negative or -inf
        const unsigned long long key = ((unsigned long long)ordered_bits(__float_as_uint(s)) << 32) | (unsigned)i;
        best = key < best ? key : best;
    }
    best = wave_min_u64(best);
    if (lane == 0) {
        a.plist[k] = p0 + (int)(best & 0xffffffffull);
        if (k == 0) *a.scount = 0;
        atomicAdd(&a.counters->pairs_transformed, 1ull);
    }
}

// ---- the rules every run kind shares (argmin, threshold, best-K) ----
// THE exclusion rule (DESIGN.md 3.2): a pair is excluded only if its lower bound, with the slack, is above its search's running
// threshold U (`gkey`, a search key; NO_KEY: none yet).  A search whose U is 1 -- no match anywhere, every score clamped to 1 --
// ties everywhere: nothing of it is excluded.  (Array and index, not the value: the bound is loaded only where U can exclude.)
__device__ __forceinline__ bool bound_excludes(const float* slb, const int pr, const unsigned long long gkey) {
    const float U = gkey == NO_KEY ? __builtin_inff() : key_score(gkey);
    return U < 0.9999f && slb[pr] > U * 1.000001f + 1e-7f;
}

// The audit of the exclusion: one search in `audit_every` is audited per run -- other ones every run --, and of it one hashed pair:
// if the bound excluded that pair, it is evaluated all the same and its bound held to what it really scores.  Whether search `k`
// (of the sub-batch) is audited in this run; which of its own pairs then; both: whether pair `pr` (of the sub-batch) is that pair.
template <class Args>
__device__ __forceinline__ bool audited_search(const Args& a, const int k) {
    return a.audit_every > 0 && ((unsigned)(a.first_search + k) + a.audit_seq) % (unsigned)a.audit_every == 0u;
}
template <class Args>
__device__ __forceinline__ int audit_pair_of(const Args& a, const SearchDesc& sd, const int k) {
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const unsigned h = ((unsigned)(a.first_search + k) * 2654435761u + a.audit_seq * 40503u) >> 9;
    return (int)(h % (unsigned)lay.n_pairs);
}
template <class Args>
__device__ __forceinline__ bool is_audit_pair(const Args& a, const int pr, const int k) {
    if (!audited_search(a, k)) return false;
    const SearchDesc sd = a.searches[k];
    return audit_pair_of(a, sd, k) == pair_of_search(a.sub_first_pair, pr, sd);
}

// the pairs `pr` of the lanes with `add` set to the end of a list, in lane order: one atomicAdd per wave (every lane calls it)
__device__ __forceinline__ void append_pairs(int* list, int* count, RunCounters* counters, const bool add, const int pr) {
    const unsigned long long m = __ballot(add);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && m) {
        base = atomicAdd(count, __popcll(m));
        atomicAdd(&counters->pairs_transformed, (unsigned long long)__popcll(m));
    }
    base = __shfl(base, 0, 64);
    if (add) list[base + __popcll(m & ((1ull << lane) - 1ull))] = pr;
}
// One reservation a WORKGROUP for the kernels that list most of what a sub-batch lists (survivor_kernel, survivor2_kernel): every
// wave of a launch adding to the same two words is a chain of same-address atomics, which serialise in the L2 (the votes' lesson,
// slb_one) -- 4.8 k of them in survivor_kernel's 0.085 ms at BASELINE configs[2].  Here the waves' counts meet in a few words of LDS
// and thread 0 reserves for all of them: `n_wave` entries of the list behind `count` for this wave -> where they begin, in wave
// order inside the workgroup; `delta_wave`, summed over the workgroup, goes to pairs_transformed (it may be negative).  Every
// thread of a workgroup of WAVES waves calls it, the arguments wave-uniform; two barriers.  A kernel that calls it again puts a
// barrier between the calls (the words are read behind the second one).
template <int WAVES>
__device__ __forceinline__ int reserve_pairs_block(int* count, RunCounters* counters, const int n_wave, const int delta_wave) {
    __shared__ int s_n[WAVES], s_delta[WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_n[w] = n_wave; s_delta[w] = delta_wave; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int before[WAVES], total = 0, delta = 0;
#pragma unroll
        for (int i = 0; i < WAVES; ++i) { before[i] = total; total += s_n[i]; delta += s_delta[i]; }
        const int base = total ? atomicAdd(count, total) : 0;
        if (delta) atomicAdd(&counters->pairs_transformed, (unsigned long long)(long long)delta);
#pragma unroll
        for (int i = 0; i < WAVES; ++i) s_n[i] = base + before[i];
    }
    __syncthreads();
    return s_n[w];
}
// append_pairs with that reservation: the same entries, in lane order inside a wave and in wave order inside the workgroup
template <int WAVES>
__device__ __forceinline__ void append_pairs_block(int* list, int* count, RunCounters* counters, const bool add, const int pr) {
    const unsigned long long m = __ballot(add);
    const int lane = threadIdx.x & 63;
    const int base = reserve_pairs_block<WAVES>(count, counters, __popcll(m), __popcll(m));
    if (add) list[base + __popcll(m & ((1ull << lane) - 1ull))] = pr;
}

// every pair but the pilots: excluded (its lower bound is above what the search has already found: pair_lb = +inf, what
// refine_kernel and collect_kernel skip by), or listed for ifft_kernel in the order of the L2-friendly schedule
// (workgroups of sixteen waves, one reservation each: 347 for the pairs of BASELINE configs[2] -- reserve_pairs_block)
constexpr int SURVIVOR_THREADS = 1024;
__global__ __launch_bounds__(SURVIVOR_THREADS)
void survivor_kernel(BoundArgs a) {
    const int b = blockIdx.x * SURVIVOR_THREADS + threadIdx.x;
    bool keep = false;
    int pr = 0;
    if (b < a.n_pairs) {
        pr = a.order[b];
        const int k = a.pairmap[pr];
        bool audit = false;
        if (a.plist[k] != pr) {
            const bool excluded = bound_excludes(a.slb, pr, a.gkeys[a.first_search + k]);
            // (is_audit_pair, from its two parts: with the flag coming back through the one helper two operands of an s_or_b64 change
            // places in this kernel's code, and the bench path's recorded counters stand on identical code; pair_of_search is
            // written out below for the same reason)
            if (excluded && audited_search(a, k)) {
                const SearchDesc sd = a.searches[k];
                audit = audit_pair_of(a, sd, k) == a.sub_first_pair + pr - sd.first_pair;
            }
            if (excluded && !audit) a.pair_lb[pr] = __builtin_inff();
            keep = !excluded || audit;
        }
        if (a.audit_mark) a.audit_mark[pr] = (audit ? MARK_AUDITED : 0) | (keep ? MARK_LISTED : 0);
    }
    append_pairs_block<SURVIVOR_THREADS / 64>(a.slist, a.scount, a.counters, keep, pr);
}

// The whole rows of the LISTED pairs, search by search (band-split form, the pairs the bound left): a workgroup = 256 consecutive
// entries of ONE search; the pattern's segment spectra go to registers once and meet the block spectra of every listed pair of
// that search in turn.  mac_list_kernel re-reads the pattern rows for every pair -- 0.6 MB a pair, 8.7 GB a step at BASELINE
// configs[2], what that kernel's time is --; here they are read once per search (1.8 GB), and the block spectra of neighbouring
// searches' pairs, walked at about the same time, meet in the L2.  Patterns of more than MAC_SMAX_LONG segments stay with
// mac_list_kernel (`long_only` there).  Same sums in the same order as mac_kernel (a segment past the pattern's end is a zero entry).
//
// An argmin run calls it TWICE (ROWS_FIRST, ROWS_REST), so that a pattern's spectra are read once for the rows known before
// anything is scored and once more only where the bound left something:
//   ROWS_FIRST, behind pilot_kernel: the search's pilot (plist[k]) and, if the search is audited in this run, its hashed audit
//     pair -- survivor_kernel lists that pair whether the bound excludes it or not, so its row can be formed while the spectra are
//     in registers.  No marks exist yet: the pairs come from the list and the hash.
//   ROWS_REST, behind the second look: the pairs marked MARK_LISTED, without the audit pair ROWS_FIRST formed (survivor_kernel has
//     rewritten the marks since: the pair is found again from the same hash arguments).  The marks are scanned BEFORE the spectra are
//     loaded, and a search with nothing left to form -- a third of the searches at BASELINE configs[2] list nothing, nearly half only
//     their audit pair -- is left at once.
//   ROWS_MARKED: every pair marked MARK_LISTED, the spectra loaded first (the route of SUSHI_HIP_PILOT_ROWS=list, where
//     mac_list_kernel forms every pilot).
//   ROWS_ITEMS: ROWS_REST's rows with another unit of work (the default; SUSHI_HIP_REST_ROWS=search: ROWS_REST).  A workgroup of
//     ROWS_REST is (search, 256 entries): more than half of them scan the marks and leave, and the real survivors sit mostly in the
//     few searches of up to four segments, whose workgroups form their rows one after the other, each a dependent round trip of six
//     loads, the multiply-accumulates and a store -- the launch ends with a few long chains on an idle chip (0.47 ms for 1.5 GB
//     at BASELINE configs[2], 3.3 TB/s where the first pass reads at 4.8).  Here a workgroup is (ITEM, 256 entries): an item is a run
//     of one search's pairs that holds at most REST_ITEM_PAIRS pairs to form (run_policy.hpp: the cut rule, and why that many),
//     listed by dense_search_kernel, which walks every search's marks anyway -- no launch more; the list is one int per item, the
//     run's first pair, in `slist` (dead once survivor2_kernel has run) and its length a word of the zeroed counters.  A fixed grid
//     strides over (item, part), the count read from device memory; the workgroup finds the search through `pairmap`, loads the
//     pattern's spectra once for the item and walks the marks on from its first pair to REST_ITEM_PAIRS pairs to form or the
//     search's end.  mac_row_of_pair is the same: every row keeps its bits.  No workgroup waits for another.
enum { ROWS_MARKED = 0, ROWS_FIRST = 1, ROWS_REST = 2, ROWS_ITEMS = 3 };
struct MacRowsArgs {
    const uint4* spec;
    int64_t spec_blocks;
    const uint4* tspec;
    int tspec_half;                   // `tspec` holds half rows (TspecLane; ROWS_FIRST then forms a row and its mirror together)
    uint4* y;
    const SearchDesc* searches;
    const TemplConsts* tconst;
    const unsigned char* mark;        // [pairs of the sub-batch] MARK_LISTED: the pair's row is formed (ROWS_FIRST: not read)
    int n_sub;
    int sub_first_seg;
    int sub_first_pair;
    const int* dense_search;          // [searches of the sub-batch]: 1 = the dense multiply-accumulate forms this search's rows instead (ROWS_FIRST: not read)
    const int* plist;                 // [searches of the sub-batch] ROWS_FIRST: the pair transformed first
    int first_search;                 // ROWS_FIRST / ROWS_REST / ROWS_ITEMS: what audited_search and audit_pair_of hash (BoundArgs' own)
    unsigned audit_seq;
    int audit_every;
    // ROWS_ITEMS
    const int* items;                 // [up to n_pairs] an item's first pair to form (a pair of the sub-batch)
    const int* item_count;            // [1] how many
    const int* pairmap;               // [pairs of the sub-batch] -> search of the sub-batch
    int n_pairs;                      // pairs of the sub-batch: the list's capacity
};
// one row: the pattern's spectra `tt` against the block spectra of pair `ip` of the search
template <int SMAX>
__device__ __forceinline__ void mac_row_of_pair(const MacRowsArgs& a, const FftLayout& lay, const sushi_mac::h8 (&tt)[SMAX],
                                                const uint4* __restrict__ zsp, const int p0, const int ip, const float sy, const int e,
                                                const int z_zero) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const long long I = lay.pair0 + ip;
    sushi_mac::acc4 acc = sushi_mac::zero_acc();
#pragma unroll
    for (int s6 = 0; s6 < SMAX; s6 += 6) {
        sushi_mac::h8 z[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const long long jj = s6 + t < lay.n_seg ? FFT_STEP * I + s6 + t : (long long)z_zero;     // (past the pattern: the zero block)
            z[t] = as_h8(zsp[(size_t)(jj < z_zero ? jj : z_zero) * ROWE]);
        }
#pragma unroll
        for (int t = 0; t < 6; ++t) {
            const sushi_mac::zrow zr = {z[t], sushi_mac::rot_mi(z[t])};
            sushi_mac::mac4(acc, tt[s6 + t], zr);
        }
    }
    unsigned o[sushi_mac::BINS];
#pragma unroll
    for (int q = 0; q < sushi_mac::BINS; ++q) {
        const h2 h = {(_Float16)(acc.re[q] * sy), (_Float16)(acc.im[q] * sy)};
        o[q] = __builtin_bit_cast(unsigned, h);
    }
    a.y[(size_t)(p0 + ip) * ROWE + e] = uint4{o[0], o[1], o[2], o[3]};
}
// ROWS_FIRST over HALF rows: a thread owns stored entry `h` of the search's half rows AND the whole-row entry that is its
// conj-reversal (fft_core.hpp half_mirror_of) -- a workgroup is 256 stored entries, eight parts a search.  The pattern's stored
// words are loaded once; they form the thread's own entry of the pilot's and the audit pair's rows as they are, and then, reversed
// and conjugated in registers, the mirrored entry of the same rows: the same sums in the same order as every other route, against
// the block spectra's entry at the mirror's index.  One after the other, so that no more loads are in flight than before.  Sixteen
// lanes' mirrors are 256 consecutive bytes in reversed lane order (the eight runs of row 0's neighbours: in two pieces): whole
// lines, read and written.  Row 0's two lanes mirror row 0 in itself: their words for it are row 1024's (reloaded in between).
template <int SMAX>
__device__ __forceinline__ void mac_rows_first_paired(const MacRowsArgs& a, const SearchDesc& sd, const FftLayout& lay, const int k,
                                                      const float sy, const int h, const int z_zero) {
    const uint4* __restrict__ hrow = a.tspec + (size_t)(sd.first_seg - a.sub_first_seg) * HROWE;
    const int e_own = sushi_fft::half_to_full(h), e_mir = sushi_fft::half_mirror_of(h);
    const int p0 = first_pair_in_sub(a.sub_first_pair, sd);
    const int audit = audited_search(a, k) ? audit_pair_of(a, sd, k) : -1;
    const int pilot = a.plist[k] - p0;
    const bool two = audit >= 0 && audit < lay.n_pairs && audit != pilot;
    sushi_mac::h8 tt[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) tt[s] = s < lay.n_seg ? as_h8(hrow[(size_t)s * HROWE + h]) : sushi_mac::zero_h8();
    mac_row_of_pair<SMAX>(a, lay, tt, a.spec + e_own, p0, pilot, sy, e_own, z_zero);
    if (two) mac_row_of_pair<SMAX>(a, lay, tt, a.spec + e_own, p0, audit, sy, e_own, z_zero);
    if ((h & ~16) == 0) {                                        // entries 0 and 1 of row 0: h = 0, 16
        const int hx = sushi_fft::half_entry(1024, h >> 4);
#pragma unroll
        for (int s = 0; s < SMAX; ++s) tt[s] = s < lay.n_seg ? as_h8(hrow[(size_t)s * HROWE + hx]) : sushi_mac::zero_h8();
    }
#pragma unroll
    for (int s = 0; s < SMAX; ++s) tt[s] = as_h8(sushi_fft::real_conjrev(as_uint4(tt[s])));
    mac_row_of_pair<SMAX>(a, lay, tt, a.spec + e_mir, p0, pilot, sy, e_mir, z_zero);
    if (two) mac_row_of_pair<SMAX>(a, lay, tt, a.spec + e_mir, p0, audit, sy, e_mir, z_zero);
}
// (`e`: the thread's entry of the whole row -- ROWS_FIRST over half rows: its stored entry of the half row)
template <int SMAX, int MODE>
__device__ __forceinline__ void mac_rows_of_search(const MacRowsArgs& a, const SearchDesc& sd, const FftLayout& lay, const int k,
                                                   const float sy, const int e, unsigned long long (*masks)[4], const int z_zero) {
    if (MODE == ROWS_FIRST && a.tspec_half) { mac_rows_first_paired<SMAX>(a, sd, lay, k, sy, e, z_zero); return; }
    const TspecLane tsp = tspec_lane(a.tspec, a.tspec_half, (size_t)(sd.first_seg - a.sub_first_seg), e);
    const uint4* __restrict__ zsp = a.spec + e;
    const int p0 = first_pair_in_sub(a.sub_first_pair, sd);
    const int tid = threadIdx.x;
    // the audit pair of the search (its index inside the search; -1: the search is not audited in this run): what ROWS_FIRST forms
    // beside the pilot and ROWS_REST leaves out
    int audit = -1;
    if (MODE != ROWS_MARKED && audited_search(a, k)) audit = audit_pair_of(a, sd, k);
    if (MODE == ROWS_REST) {
        bool any = false;
        for (int i = tid; i < lay.n_pairs; i += MACL_THREADS) any = any || (i != audit && (a.mark[p0 + i] & MARK_LISTED));
        if (!__syncthreads_or(any)) return;                    // (uniform: nothing of this search is left to form)
    }
    sushi_mac::h8 tt[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) tt[s] = s < lay.n_seg ? as_h8(tspec_entry(tsp, (size_t)s)) : sushi_mac::zero_h8();
    if (MODE == ROWS_FIRST) {
        const int pilot = a.plist[k] - p0;
        mac_row_of_pair<SMAX>(a, lay, tt, zsp, p0, pilot, sy, e, z_zero);
        if (audit >= 0 && audit < lay.n_pairs && audit != pilot) mac_row_of_pair<SMAX>(a, lay, tt, zsp, p0, audit, sy, e, z_zero);
        return;
    }
    for (int base = 0; base < lay.n_pairs; base += MACL_THREADS) {
        // which of these 256 pairs are listed: one flag per thread, a ballot per wave
        __syncthreads();
        const int i = base + tid;
        const bool on = i < lay.n_pairs && (MODE == ROWS_MARKED || i != audit) && (a.mark[p0 + i] & MARK_LISTED);
        const unsigned long long bm = __ballot(on);
        if ((tid & 63) == 0) (*masks)[tid >> 6] = bm;
        __syncthreads();
        for (int w = 0; w < 4; ++w) {
            unsigned long long m = (*masks)[w];
            while (m) {
                const int bit = __builtin_ctzll(m);
                m &= m - 1;
                mac_row_of_pair<SMAX>(a, lay, tt, zsp, p0, base + 64 * w + bit, sy, e, z_zero);
            }
        }
    }
}
// ROWS_ITEMS: the rows of one item, the run of the search's pairs that starts at its pair `first` (a pair to form).  Every wave
// reads the same marks and takes the same pairs: no exchange, no barrier.
template <int SMAX>
__device__ __forceinline__ void mac_rows_of_item(const MacRowsArgs& a, const SearchDesc& sd, const FftLayout& lay, const int k,
                                                 const float sy, const int e, const int z_zero, const int first) {
    const TspecLane tsp = tspec_lane(a.tspec, a.tspec_half, (size_t)(sd.first_seg - a.sub_first_seg), e);
    const uint4* __restrict__ zsp = a.spec + e;
    const int p0 = first_pair_in_sub(a.sub_first_pair, sd);
    const int audit = audited_search(a, k) ? audit_pair_of(a, sd, k) : -1;
    sushi_mac::h8 tt[SMAX];
#pragma unroll
    for (int s = 0; s < SMAX; ++s) tt[s] = s < lay.n_seg ? as_h8(tspec_entry(tsp, (size_t)s)) : sushi_mac::zero_h8();
    int room = REST_ITEM_PAIRS;
    for (int base = first; base < lay.n_pairs && room > 0; base += 64) {
        const int i = base + (threadIdx.x & 63);
        const bool on = i < lay.n_pairs && rest_pair_to_form(a.mark[p0 + i] & MARK_LISTED, i, audit);
        unsigned long long m = rest_item_take(__ballot(on), room);
        room -= __popcll(m);
        while (m) {
            const int bit = __builtin_ctzll(m);
            m &= m - 1;
            mac_row_of_pair<SMAX>(a, lay, tt, zsp, p0, base + bit, sy, e, z_zero);
        }
    }
}
// LONG 0: patterns of up to MAC_SMAX_SHORT segments; 1: longer ones up to MAC_SMAX_LONG (their registers halve the occupancy)
template <int LONG, int MODE>
__global__ __launch_bounds__(MACL_THREADS)
void mac_rows_kernel(MacRowsArgs a) {
    __shared__ unsigned long long masks[4];
    const int z_zero = (int)(a.spec_blocks < 0x7fffffff ? a.spec_blocks : 0x7fffffff);
    if (MODE == ROWS_ITEMS) {
        const int listed = *a.item_count;
        const int n_items = listed < a.n_pairs ? listed : a.n_pairs;           // (the list's capacity)
        for (long long it = blockIdx.x; it < (long long)n_items * MACL_PARTS; it += gridDim.x) {
            const int first = __builtin_amdgcn_readfirstlane(a.items[it / MACL_PARTS]);
            if ((unsigned)first >= (unsigned)a.n_pairs) continue;
            const int k = __builtin_amdgcn_readfirstlane(a.pairmap[first]);
            if ((unsigned)k >= (unsigned)a.n_sub || a.dense_search[k]) continue;   // (the dense multiply-accumulate forms this search's rows)
            const int e = (int)(it % MACL_PARTS) * MACL_THREADS + threadIdx.x;
            const SearchDesc sd = a.searches[k];
            const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
            const float sy = a.tconst[k].mac_scale;
            const int i0 = first - first_pair_in_sub(a.sub_first_pair, sd);
            if ((unsigned)i0 >= (unsigned)lay.n_pairs) continue;
            if (LONG) {
                if (lay.n_seg > MAC_SMAX_SHORT && lay.n_seg <= MAC_SMAX_LONG) mac_rows_of_item<MAC_SMAX_LONG>(a, sd, lay, k, sy, e, z_zero, i0);
            } else {
                if (lay.n_seg <= 6) mac_rows_of_item<6>(a, sd, lay, k, sy, e, z_zero, i0);
                else if (lay.n_seg <= 12) mac_rows_of_item<12>(a, sd, lay, k, sy, e, z_zero, i0);
                else if (lay.n_seg <= MAC_SMAX_SHORT) mac_rows_of_item<MAC_SMAX_SHORT>(a, sd, lay, k, sy, e, z_zero, i0);
            }
        }
        return;
    }
    // (ROWS_FIRST over half rows: a workgroup is 256 STORED entries, half as many parts a search -- mac_rows_first_paired)
    const int parts = MODE == ROWS_FIRST && a.tspec_half ? MACL_PARTS / 2 : MACL_PARTS;
    for (long long it = blockIdx.x; it < (long long)a.n_sub * parts; it += gridDim.x) {
        const int k = (int)(it / parts);
        if (MODE != ROWS_FIRST && a.dense_search[k]) continue;  // (uniform: a workgroup is one search's)
        const int e = (int)(it % parts) * MACL_THREADS + threadIdx.x;
        const SearchDesc sd = a.searches[k];
        const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
        const float sy = a.tconst[k].mac_scale;
        if (LONG) {
            if (lay.n_seg > MAC_SMAX_SHORT && lay.n_seg <= MAC_SMAX_LONG) mac_rows_of_search<MAC_SMAX_LONG, MODE>(a, sd, lay, k, sy, e, &masks, z_zero);
        } else {
            if (lay.n_seg <= 6) mac_rows_of_search<6, MODE>(a, sd, lay, k, sy, e, &masks, z_zero);
            else if (lay.n_seg <= 12) mac_rows_of_search<12, MODE>(a, sd, lay, k, sy, e, &masks, z_zero);
            else if (lay.n_seg <= MAC_SMAX_SHORT) mac_rows_of_search<MAC_SMAX_SHORT, MODE>(a, sd, lay, k, sy, e, &masks, z_zero);
        }
        // (longer patterns still: mac_list_kernel, several passes)
    }
}

// A SECOND LOOK at the pairs the band-split bound left (a few per cent of all; most of them belong to the shortest patterns, whose
// match stands least above what chance correlates: profiles/r05/dev/survivor_stats_*.txt).  bound_low_kernel bounds the low band's
// samples by a Cauchy-Schwarz sum over its eight decimated groups; here the N/2 samples themselves are formed -- one 8192-point
// float32 transform of the low row (fft_core.hpp Plan<13>), bin 0 out and signed as there -- and their largest modulus taken: the
// sharpest the sampling bound gets.  slb_list_kernel then redoes the pair's lower bound and survivor2_kernel drops what it now
// excludes, before any whole row is formed.  ~25 ns a listed pair against ~130 for its whole row and transform.
constexpr int BLE_LOGN = 13;
constexpr int BLE_N = sushi_fft::Plan<BLE_LOGN>::N, BLE_T = sushi_fft::Plan<BLE_LOGN>::NT;
static_assert(BLE_N == FN / 2, "the low band sampled at every second position");
// sqrt(2) x the largest sample (`mm`: its square as float bits) + bin 0's own part, signed.  The float32 transform's own error is at
// most 1e-5 of the inputs' sum of moduli <= 1e-5 sqrt(4096) |inputs|_2 = 1e-5 sqrt(4096 / 8192) |outputs|_2 <= 6.4e-4 x the largest
// output (Parseval over the 8192 samples): a factor, not a term that needs the row's energy
__device__ __forceinline__ float second_look_bound(const unsigned mm, const float dc_re, const float dc_im) {
    const float bw = 1.4142137f * sqrtf(__uint_as_float(mm)) * 1.0007f + fmaxf(dc_re, dc_im);
    return mm >= 0x7f800000u ? __builtin_inff() : bw;
}
// The kernel's fixed costs per slot are what it runs on (~1200 slots a launch at BASELINE configs[2], one or two a workgroup):
//   * which of a thread's sixteen input registers lie in the band depends on the register alone, and the eight that do are two
//     16-byte entries of the row (fft_core.hpp sl_in_band, sl_sub, sl_entry): two loads, the other eight registers constants;
//   * the next slot's two entries (and the pair after that one) are requested before the current slot is transformed;
//   * the largest sample meets in ONE word of LDS -- float bits of squares order as unsigned --, an atomic a wave, one barrier:
//     the word of the next slot is cleared in front of that barrier, the two words taking turns.
// The same loads' values, fft_split as it is, the same maximum: acc[2 pr] keeps its bits (SUSHI_HIP_SECOND_LOOK=plain: the body
// before this one, bound_low_exact_plain_kernel below, for A/B runs on one build).
__global__ __launch_bounds__(BLE_T, 8)                          // (eight waves a SIMD -- four workgroups a CU, as the buffer allows: 64 registers)
void bound_low_exact_kernel(BoundArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[sushi_fft::lds_floats<BLE_LOGN>()];
    __shared__ unsigned red[2];
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const int n = *a.list_count;
    if (n > a.n_pairs / 5) return;
    int slot = blockIdx.x;
    if (slot >= n) return;
    if (threadIdx.x == 0) { red[0] = 0u; red[1] = 0u; }          // (fft_split's barriers lie between this and the first atomic)
    const sushi_fft::uint4v* __restrict__ rows = reinterpret_cast<const sushi_fft::uint4v*>(a.y);
    int pr = a.list[slot];
    sushi_fft::uint4v w0, w1;
    {
        const int t0 = threadIdx.x;
        w0 = rows[(size_t)pr * LROWE + sushi_fft::sl_entry(t0, 0)]; w1 = rows[(size_t)pr * LROWE + sushi_fft::sl_entry(t0, 1)];
    }
    int slot_n = slot + gridDim.x;
    int pr_n = slot_n < n ? a.list[slot_n] : pr;                 // (the last slot re-requests itself: unconditional loads)
    for (int turn = 0;; turn ^= 1) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));                            // (per-iteration constants stay inside the iteration: hoisted, they spill)
        const sushi_fft::uint4v n0 = rows[(size_t)pr_n * LROWE + sushi_fft::sl_entry(tid, 0)];
        const sushi_fft::uint4v n1 = rows[(size_t)pr_n * LROWE + sushi_fft::sl_entry(tid, 1)];
        const int slot_nn = slot_n + gridDim.x;
        const int pr_nn = slot_nn < n ? a.list[slot_nn] : pr_n;
        const float first_look = tid == 0 ? a.acc[2 * (size_t)pr] : 0.f;
        const sushi_fft::Twiddles tw = sushi_fft::load_twiddles<BLE_LOGN, 1>(tid, twiddles());
        __builtin_amdgcn_sched_barrier(0);                       // (the requests stay in front of the transform)
        cpx v[sushi_fft::PER];
#pragma unroll
        for (int r = 0; r < sushi_fft::PER; ++r) {
            if (sushi_fft::sl_in_band(r)) {
                const h2 h = __builtin_bit_cast(h2, r < 8 ? w0[sushi_fft::sl_sub(r)] : w1[sushi_fft::sl_sub(r)]);
                v[r] = cpx{(float)h.x, (float)h.y};
            } else {
                v[r] = cpx{0.f, 0.f};
            }
        }
        float dc_re = 0.f, dc_im = 0.f;
        if (tid == 0) { dc_re = v[0].x; dc_im = v[0].y; v[0] = cpx{0.f, 0.f}; }       // (bin 0: register 0 of thread 0)
        sushi_fft::fft_split<BLE_LOGN, 1>(v, tid, lds, tw);
        float m2 = 0.f;
#pragma unroll
        for (int r = 0; r < sushi_fft::PER; ++r) m2 = fmaxf(m2, v[r].x * v[r].x + v[r].y * v[r].y);
        const unsigned wm = wave_max_u32(__float_as_uint(m2));
        if ((tid & 63) == 0) atomicMax(&red[turn], wm);
        if (tid == 0) red[turn ^ 1] = 0u;
        __syncthreads();                                         // (also the barrier the transform's buffer needs before its next use)
        // (never above the first look's: both are bounds)
        if (tid == 0) a.acc[2 * (size_t)pr] = fminf(first_look, second_look_bound(red[turn], dc_re, dc_im));
        slot = slot_n;
        if (slot >= n) break;
        pr = pr_n; w0 = n0; w1 = n1; slot_n = slot_nn; pr_n = pr_nn;
    }
}
// the body before that one (SUSHI_HIP_SECOND_LOOK=plain)
__global__ __launch_bounds__(BLE_T)
void bound_low_exact_plain_kernel(BoundArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[sushi_fft::lds_floats<BLE_LOGN>()];
    __shared__ unsigned red[BLE_T / 64];
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const int n = *a.list_count;
    if (n > a.n_pairs / 5) return;
    for (int slot = blockIdx.x; slot < n; slot += gridDim.x) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));                            // (per-iteration constants stay inside the iteration)
        const sushi_fft::Twiddles tw = sushi_fft::load_twiddles<BLE_LOGN, 1>(tid, twiddles());
        const int pr = a.list[slot];
        const uint32_t* __restrict__ row = reinterpret_cast<const uint32_t*>(a.y) + (size_t)pr * (LROWE * 4);
        cpx v[sushi_fft::PER];
        float dc_re = 0.f, dc_im = 0.f;
#pragma unroll
        for (int r = 0; r < sushi_fft::PER; ++r) {
            const int kin = sushi_fft::in_index<BLE_LOGN>(tid, r);        // index on the N/2 grid: the band is kin < N/8 and kin >= 3N/8
            const bool in_band = kin < FN / 8 || kin >= 3 * FN / 8;
            const int ls = sushi_fft::lslot_of_bin(kin < FN / 8 ? kin : (in_band ? kin + FN / 2 : 0));
            const h2 h = __builtin_bit_cast(h2, in_band ? row[ls] : 0u);
            v[r] = cpx{(float)h.x, (float)h.y};
            if (kin == 0) { dc_re = v[r].x; dc_im = v[r].y; v[r] = cpx{0.f, 0.f}; }
        }
        sushi_fft::fft_split<BLE_LOGN, 1>(v, tid, lds, tw);
        float m2 = 0.f;
#pragma unroll
        for (int r = 0; r < sushi_fft::PER; ++r) m2 = fmaxf(m2, v[r].x * v[r].x + v[r].y * v[r].y);
        const unsigned wm = wave_max_u32(__float_as_uint(m2));
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = wm;
        __syncthreads();
        if (tid == 0) {
            unsigned mm = 0u;
#pragma unroll
            for (int i = 0; i < BLE_T / 64; ++i) mm = red[i] > mm ? red[i] : mm;
            // sqrt(2) x the largest sample + bin 0's own part, signed.  The float32 transform's own error is at most 1e-5 of the inputs'
            // sum of moduli <= 1e-5 sqrt(4096) |inputs|_2 = 1e-5 sqrt(4096 / 8192) |outputs|_2 <= 6.4e-4 x the largest output
            // (Parseval over the 8192 samples): a factor, not a term that needs the row's energy
            float bw = 1.4142137f * sqrtf(__uint_as_float(mm)) * 1.0007f + fmaxf(dc_re, dc_im);
            if (mm >= 0x7f800000u) bw = __builtin_inff();
            // (never above the first look's: both are bounds)
            a.acc[2 * (size_t)pr] = fminf(a.acc[2 * (size_t)pr], bw);
        }
        __syncthreads();
    }
}
// ... and what the second look leaves: the list again, without the pairs whose new bound excludes them
__global__ __launch_bounds__(256)
void survivor2_kernel(BoundArgs a) {
    const int n = *a.list_count;
    const bool second_look = n <= a.n_pairs / 5;
    for (int base = blockIdx.x * 256; base < n; base += gridDim.x * 256) {
        const int slot = base + threadIdx.x;
        bool keep = false;
        int pr = 0;
        if (slot < n) {
            pr = a.list[slot];
            keep = true;
            if (second_look && !(a.audit_mark[pr] & MARK_AUDITED)) {
                const int k = a.pairmap[pr];
                if (bound_excludes(a.slb, pr, a.gkeys[a.first_search + k])) {
                    // the audit of THIS bound: a hashed sample of the pairs it excludes -- other ones every run -- stays listed, is
                    // transformed all the same, and ifft_kernel holds the pair's (second) lower bound to what it really scores
                    const unsigned h = ((unsigned)(a.sub_first_pair + pr) * 2654435761u + a.audit_seq * 40503u) >> 11;
                    if (a.audit_every > 0 && h % (16u * (unsigned)a.audit_every) == 0u) {
                        a.audit_mark[pr] = MARK_AUDITED | MARK_LISTED | MARK_SECOND_LOOK;
                    } else {
                        keep = false;
                        a.pair_lb[pr] = __builtin_inff();
                        a.audit_mark[pr] = 0;
                    }
                }
            }
        }
        const unsigned long long m = __ballot(keep), act = __ballot(slot < n);
        const int lane = threadIdx.x & 63;
        const int dropped = __popcll(act) - __popcll(m);          // (they were counted as transformed when they were listed)
        const int b0 = reserve_pairs_block<4>(a.list2_count, a.counters, __popcll(m), -dropped);
        if (keep) a.list2[b0 + __popcll(m & ((1ull << lane) - 1ull))] = pr;
        __syncthreads();                                           // (a further round writes the reservation's words again)
    }
}

// Band-split form, after the survivors are known: forming whole rows pair by pair (mac_rows_kernel / mac_list_kernel, ~120 ns a
// listed pair) beats the dense multiply-accumulate only while few pairs are listed.  The dense form's unit of work is an ITEM --
// eight searches of one class whose windows lie next to each other, walked together by every wave (~25 us at BASELINE configs[2],
// whatever its members need, and more when few items run: neighbouring items share their rows in the L2): listed pairs x 120 ns
// against a search's eighth of an item comes to two ninths of its pairs; measured, 6 dB of noise (short patterns with dozens of
// survivors, 8 % of all pairs listed) is better off pair by pair and a dub (its own speech: every pair of such a search listed) in
// the dense form: the line is drawn at two fifths.  Decided per SEARCH since round 6, and the searches that take the dense form are
// REGROUPED into items of their own (dense_repack_kernel): a dub's searches under speech alternate with searches under the shared
// music bed, every item of the plan mixes the two, and the per-item decision of before formed whole rows for all eight members of
// nearly every item -- four ninths of that work for searches that needed two or three rows (bench.py --source dub: 24.1 -> 21.5 ms).
// (Per search WITHOUT regrouping was round 5's first try: a lone dense search cost a whole 25 us item, 0.8 ms a step.)  And the
// dense form is taken only when the searches that want it hold an eighth of the sub-batch's pairs between them (dense_repack_kernel
// clears their marks otherwise): a handful of items on an otherwise empty chip run at a fraction of a full launch's rate -- the
// short patterns of BASELINE configs[2] whose survivors exceed two fifths of their pairs (1 - 2 % of all pairs) cost 1.4 ms a step
// in the dense form, the ones at 6 dB of noise (2 - 9 %) 1.4 ms more than pair by pair.
__global__ __launch_bounds__(64)
void dense_search_kernel(BoundArgs a, int* __restrict__ dense_search, int* __restrict__ any, int* __restrict__ items,
                         int* __restrict__ item_count) {
    const int lane = threadIdx.x;
    const int k = blockIdx.x;
    const SearchDesc sd = a.searches[k];
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const int p0 = first_pair_in_sub(a.sub_first_pair, sd);
    // `items` (or NULL): the work items of mac_rows_kernel's ROWS_ITEMS pass (its header) -- the search's pairs to form, cut by
    // run_policy.hpp's rule, each item the sub-batch index of its first pair; whatever becomes of the dense flags later, the
    // consumer skips the searches that keep theirs.  One atomicAdd per 64 pairs that start an item; the list holds a slot per pair.
    const int audit = items && audited_search(a, k) ? audit_pair_of(a, sd, k) : -1;
    int listed = 0, formed = 0;
    for (int base = 0; base < lay.n_pairs; base += 64) {
        const int i = base + lane;
        const int on = i < lay.n_pairs ? (a.audit_mark[p0 + i] & MARK_LISTED) : 0;
        listed += on ? 1 : 0;
        if (items) {
            const unsigned long long form = __ballot(rest_pair_to_form(on, i, audit));
            const unsigned long long starts = rest_item_starts(form, formed, REST_ITEM_PAIRS);
            formed += __popcll(form);
            if (starts) {
                int slot = 0;
                if (lane == 0) slot = atomicAdd(item_count, __popcll(starts));
                slot = __shfl(slot, 0, 64) + __popcll(starts & ((1ull << lane) - 1ull));
                if (((starts >> lane) & 1ull) && slot < a.n_pairs) items[slot] = p0 + i;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) listed += __shfl_xor(listed, d, 64);
    if (lane == 0) {
        const int dense = listed * 5 > lay.n_pairs * 2 ? 1 : 0;
        dense_search[k] = dense;
        if (dense) atomicAdd(any, listed);                       // listed pairs of the searches that would take the dense form
    }
}

// The dense searches of an item list (workgroup 0: mac_kernel's, workgroup 1: mac_long_kernel's), class by class in the order the
// plan holds them (window start), eight to a new item: `out` has the list's own number of slots, filled from the front, the rest
// marked class -1 (the workgroups of such a slot leave at once).  Nothing to do -- the usual case -- when no search is dense (*any
// == 0: the launch that would read `out` is called off by the same flag).
constexpr int REPACK_THREADS = 1024;
__global__ __launch_bounds__(REPACK_THREADS)
void dense_repack_kernel(const int* __restrict__ items0, int n_items0, const int* __restrict__ items1, int n_items1,
                         int* __restrict__ dense_search, int n_search, int* __restrict__ out0, int* __restrict__ out1,
                         const int* __restrict__ listed_dense, int min_listed, int* __restrict__ any) {
    // too few for the dense form to pay (a handful of items on an empty chip run at a fraction of the rate of a full launch): pair by pair after all
    if (*listed_dense < min_listed) {
        if (blockIdx.x == 0) for (int k = threadIdx.x; k < n_search; k += REPACK_THREADS) dense_search[k] = 0;
        return;
    }
    if (threadIdx.x == 0) *any = 1;
    const int* __restrict__ items = blockIdx.x == 0 ? items0 : items1;
    const int n_items = blockIdx.x == 0 ? n_items0 : n_items1;
    int* __restrict__ out = blockIdx.x == 0 ? out0 : out1;
    if (n_items == 0) return;
    __shared__ int wave_tot[REPACK_THREADS / 64];
    __shared__ int carry_s, out_base_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < n_items * (1 + MAC_SPW); e += REPACK_THREADS) out[e] = -1;
    if (tid == 0) out_base_s = 0;
    __syncthreads();
    const int n_ent = n_items * MAC_SPW;
    for (int c = 0; c < MAC_CLASSES; ++c) {
        if (tid == 0) carry_s = 0;
        __syncthreads();
        for (int e0 = 0; e0 < n_ent; e0 += REPACK_THREADS) {
            const int e = e0 + tid;
            int member = -1;
            if (e < n_ent) {
                const int* __restrict__ item = items + (size_t)(e / MAC_SPW) * (1 + MAC_SPW);
                const int k = item[1 + e % MAC_SPW];
                if (item[0] == c && k >= 0 && dense_search[k] != 0) member = k;
            }
            const unsigned long long m = __ballot(member >= 0);
            if (lane == 0) wave_tot[wave] = __popcll(m);
            __syncthreads();
            int before = carry_s;
            for (int w = 0; w < wave; ++w) before += wave_tot[w];
            if (member >= 0) {
                const int pos = before + __popcll(m & ((1ull << lane) - 1ull));
                int* __restrict__ o = out + (size_t)(out_base_s + pos / MAC_SPW) * (1 + MAC_SPW);
                o[1 + pos % MAC_SPW] = member;
                if (pos % MAC_SPW == 0) o[0] = c;
            }
            __syncthreads();
            if (tid == 0) { int t = 0; for (int w = 0; w < REPACK_THREADS / 64; ++w) t += wave_tot[w]; carry_s += t; }
            __syncthreads();
        }
        if (tid == 0) out_base_s += (carry_s + MAC_SPW - 1) / MAC_SPW;
        __syncthreads();
    }
}
