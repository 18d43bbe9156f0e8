// sushi_amd/csrc/sushi_fft_ifft.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// the inverse transform of a block pair with its fused scoring epilogue, the pair's error model, candidates and audit runs.

// ------------------------------------------------------------------------------------------
// Inverse transform of one block pair + fused scoring epilogue
// ------------------------------------------------------------------------------------------
struct IfftArgs {
    const uint2* y;                   // [pairs of the sub-batch][FN / 2]: the products as packed halves
    const double* dst_stats;          // [1]: the constant the block spectra are centred by
    const SearchDesc* searches;       // the sub-batch's searches
    int n_sub;
    int first_search;                 // global index of searches[0]
    int sub_first_pair;
    int64_t dst_len;
    float delta;
    unsigned long long* cand;         // [pairs of the sub-batch][FFT_ROW]
    float* pair_lb;                   // [pairs of the sub-batch] smallest lower bound (score - e) of the pair: what refine_kernel scans
    unsigned long long* gkeys;        // [all searches] running minimum of (f32 score + error bound)
    const int* pairmap;               // [pairs of the sub-batch] -> search index inside the sub-batch
    const int* order;                 // [pairs of the sub-batch] workgroup -> pair (L2-friendly schedule; or a list of pairs), or NULL
    const int* count;                 // NULL, or how many entries of `order` exist: workgroups beyond leave at once
    const TemplConsts* tconst;        // [searches of the sub-batch]
    const float* urel;                // dst stream: prefix of the uncentred squares relative to its block's base
    const double* ubase;              // dst stream: those block bases [nb + 1]
    const float* usrel;               // dst stream: (urel, prefix of the samples relative to its block's base) interleaved (TM_CCOEFF_NORMED)
    const double* sbase;              // dst stream: those block bases [nb + 1]
    int64_t nb;                       // blocks of the dst stream
    // collection pass only
    const int* flags;                 // [all searches] 1 = list the candidates, 2 = every position
    const int* flag_list;             // flagged searches of this sub-batch (global indices)
    SubCounters* sub;                 // this sub-batch's counters (sub_flagged: how many; collect_kernel's tile list and candidate buffer heads)
    const int* citems;                // the (flagged search, pair) items refine_kernel listed: pair indices inside the sub-batch
    const int* n_citems;              // [1] how many
    TileDesc* tiles;
    int32_t* candbuf;
    int cand_cap;
    RunCounters* counters;
    // the audit of the exclusion: every transformed pair's lower bound against what the pair really scores
    const float* slb;                 // [pairs of the sub-batch] or NULL (no exclusion in this run)
    const unsigned char* audit_mark;  // [pairs of the sub-batch] MARK_AUDITED = the bound had EXCLUDED this pair (transformed as a check)
    int* viol;                        // [all searches] set to 1 where a lower bound turns out above a real score
    int list_first;                   // with `count`: the first list slot this launch takes ...
    int list_direct;                  // ... one workgroup per slot (ifft_kernel), or a fixed grid striding from there on (ifft_list_kernel)
};

constexpr int GQ = 4;                      // positions per window-energy load group
static_assert(GQ % 2 == 0 && HPT % (GQ / 2) == 0, "a load group is GQ / 2 positions of both halves");

// Everything the epilogue of one pair needs, per thread.  Scores are indexed half * HPT + r for position
// pos = half * FH + tid + FT * r of the pair.  A score is what the ranking MINIMISES: the TM_SQDIFF_NORMED value itself,
// or 1 - the TM_CCOEFF_NORMED value (arg-max as an arg-min, in [0, 2]).  Positions outside the search hold +inf;
// TM_CCOEFF_NORMED positions whose window variance is inside its own f32 rounding error ("uncertain": flat or nearly
// flat windows, whose score the f32 stage cannot bound) hold UNCERTAIN: always candidates, never part of the pair's minimum.
constexpr float UNCERTAIN = -1.0f;
struct PairScores {
    float scores[2 * HPT];
    float best;          // smallest score of this thread (uncertain positions aside)
    float max_rs;        // largest 1 / sqrt(window energy | window variance sum) over this thread's valid, certain positions
    int any_uncertain;
};

// constants of the TM_CCOEFF_NORMED error model (DESIGN.md 3.2), in units of eps = 2^-24:
//   numerator   sum (T - mean T) I : |err| <= eps * |T_c| * |Z| * FFT_KE   (the cross term of the centred pattern as it is)
//   variance    wU - wS1^2 / M     : |err| <= eps * |Z|^2 * CD,  CD = 28 + 512 / sqrt(M)
// (|Z|^2 = the energy of the samples that enter the pair's transforms; window sums come from float32 prefix values
// relative to per-block float64 bases: each of them is off by <= eps * 64 |Z|, wS1 <= sqrt(M) |Z|, tmean <= |T| / sqrt(M)).
__device__ __forceinline__ float ccoeff_cd(float inv_sqrt_m) { return 28.0f + 512.0f * inv_sqrt_m; }

// Y of one pair (packed halves) into the registers of the inverse transform.  Y is stored in the order the transform loads
// it: one 16-byte load brings four registers, a wave's load instruction one contiguous KiB.  Issued before anything else a
// workgroup does: the address needs the pair index only, and the search's descriptor and constants (two more dependent
// loads) are not needed before the epilogue -- with two workgroups per CU every serial hop at a workgroup's start is CU time.
__device__ __forceinline__ float load_y(sushi_fft::uint4v (&yl)[4], const uint2* __restrict__ yin, const int tid) {
    const sushi_fft::uint4v* __restrict__ yh = reinterpret_cast<const sushi_fft::uint4v*>(yin);
    float q2 = 0.f;                                              // energy of this thread's part of the row (quantisation model)
#pragma unroll
    for (int u = 0; u < sushi_fft::PER / 4; ++u) {
        yl[u] = yh[sushi_fft::wslot_uint4(tid, u)];              // four bins: eight halves, as they go to the matrix pipe
        q2 = add_abs2_entry(yl[u], q2);                          // |Y(f)|^2 straight from the halves
    }
    return q2;
}

// One pair: inverse transform of the loaded Y, f32 scores.  Returns through `ps`; `plo`/`phi` bound the valid positions.
// METHOD 0  score = sum (T - I)^2 / sqrt(sum T^2 * sum I^2), everything UNCENTRED: the f32 error of the FFT'd cross term
//           is then bounded by FFT_KE * eps * |T| * |Z| (sushi_common.hpp), i.e. in score units 2 * FFT_KE * eps * |Z| / |window|.
// METHOD 1  score = 1 - (sum T I - sum I * mean T) / sqrt(sum (T - mean T)^2 * (sum I^2 - (sum I)^2 / M)): the same cross
//           term with the same bound; the window sums come from the stream's second relative prefix (srel / sbase).
template <int METHOD>
__device__ __forceinline__ void score_pair(const IfftArgs& a, const sushi_fft::uint4v (&yl)[4], const sushi_fft::MfmaB& mb, const SearchDesc& sd,
                                           const TemplConsts& tc, const int64_t pairI, float* lds, const int tid,
                                           const sushi_fft::WTwiddles& tw, PairScores& ps, int& plo_out, int& phi_out,
                                           float& zn_out, float& znc_out) {
    constexpr bool CC = METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED;
    constexpr int GQM = CC ? GQ / 2 : GQ;                        // METHOD 1 holds two values per window end: half as many positions per group
    constexpr int NG = 2 * HPT / GQM;
    const int M = sd.tmpl_len;
    const int64_t P = sd.n_pos;
    const int64_t w = sd.win_start;
    const int64_t n = a.dst_len;
    const int64_t kA = pairI * FFT_STEP;                         // first block of the pair
    const int64_t qbase = kA * FFT_SEG;                          // dst sample of this pair's first position
    // Window energies come from the stream's block-relative prefix of squares: two 4-byte loads per
    // position (urel[q], urel[q + M]), requested group by group just ahead of the scoring of that group.
    // Positions qbase + pos: scalar base + 32-bit lane offsets; offsets past the end of the stream are
    // clamped so that the loads stay unconditional (such positions are masked below).
    const float* __restrict__ r0b = a.urel + qbase;
    const int64_t room = n - qbase;                                      // urel has n + 1 entries
    const int lim0 = (int)(room < 2 * FH - 1 ? room : 2 * FH - 1);
    const int64_t roomM = room - M;
    const int limM = (int)(roomM < 2 * FH - 1 ? roomM : 2 * FH - 1);     // may be negative
    const float* __restrict__ rMb = limM < 0 ? r0b : r0b + M;
    const int limMc = limM < 0 ? 0 : limM;
    typedef float f2v __attribute__((ext_vector_type(2)));
    const f2v* __restrict__ s0b = reinterpret_cast<const f2v*>(a.usrel) + qbase;      // (METHOD 1) both prefixes, interleaved: one 8-byte load per end
    const f2v* __restrict__ sMb = limM < 0 ? s0b : s0b + M;
    float ra[GQM], rb[GQM], ra_n[GQM], rb_n[GQM];
    float sa[CC ? GQM : 1], sb_[CC ? GQM : 1], sa_n[CC ? GQM : 1], sb_n[CC ? GQM : 1];
    unsigned after_fft = 0;
    const int Mh = M / FFT_SEG, Ml = M - Mh * FFT_SEG;
    // A pair whose 2H positions are all result positions of the search and all loadable (every pair but
    // the first and last of a window, and those at the end of the stream) takes the `interior` variants:
    // immediate load offsets, no clamps, no validity masks.
    const int64_t plo64 = w - qbase;
    const int plo = (int)(plo64 < -1 ? -1 : plo64);              // valid positions: plo <= pos < phi
    const int64_t phi64 = P + (w - qbase);
    const int phi = (int)(phi64 < 2 * FH ? phi64 : 2 * FH);
    const bool interior = lim0 >= 2 * FH - 1 && limM >= 2 * FH - 1 && plo <= 0 && phi >= 2 * FH;
    plo_out = plo; phi_out = phi;
    // Load group g = positions r = (GQM/2) g .. (GQM/2) g + GQM/2 - 1 of BOTH halves: once a group is scored, the transform
    // outputs it used are dead (v[r].x is half 0's cross term, v[r].y half 1's).
    auto load_group = [&](const int g, float (&xa)[GQM], float (&xb)[GQM], float (&ya)[CC ? GQM : 1], float (&yb)[CC ? GQM : 1],
                          auto interior_tag) {
        constexpr bool INTERIOR = decltype(interior_tag)::value;
#pragma unroll
        for (int q = 0; q < GQM; ++q) {
            const int r = g * (GQM / 2) + q / 2;
            const int half = q & 1;
            const int pos = tid + FT * r + half * FH;
            if (INTERIOR) {
                // each load's base is an opaque scalar: left visible, base + lane offset is shared between the loads and
                // every displacement past the instruction's 4 KB immediate costs a 64-bit vector add
                if (CC) {
                    typedef const __attribute__((address_space(1))) f2v* gptr2;
                    gptr2 qa = (gptr2)(s0b + FT * r + half * FH);
                    gptr2 qb = (gptr2)(sMb + FT * r + half * FH);
                    asm volatile("" : "+s"(qa));
                    asm volatile("" : "+s"(qb));
                    const f2v va = qa[(unsigned)(tid + after_fft) & 0x7fffu];
                    const f2v vb = qb[(unsigned)(tid + after_fft) & 0x7fffu];
                    xa[q] = va.x; ya[q] = va.y;
                    xb[q] = vb.x; yb[q] = vb.y;
                } else {
                    typedef const __attribute__((address_space(1))) float* gptr;
                    gptr pa = (gptr)(r0b + FT * r + half * FH);
                    gptr pb = (gptr)(rMb + FT * r + half * FH);
                    asm volatile("" : "+s"(pa));
                    asm volatile("" : "+s"(pb));
                    xa[q] = pa[(unsigned)(tid + after_fft) & 0x7fffu];
                    xb[q] = pb[(unsigned)(tid + after_fft) & 0x7fffu];
                }
            } else {
                const unsigned oa = (((unsigned)(pos <= lim0 ? pos : lim0)) + after_fft) & 0x7fffu;
                const unsigned ob = (((unsigned)(pos <= limM ? pos : limMc)) + after_fft) & 0x7fffu;
                if (CC) {
                    const f2v va = s0b[oa], vb = sMb[ob];
                    xa[q] = va.x; ya[q] = va.y;
                    xb[q] = vb.x; yb[q] = vb.y;
                } else {
                    xa[q] = r0b[oa];
                    xb[q] = rMb[ob];
                }
            }
        }
    };
    // The block bases sit at wave-uniform addresses: scalar loads into SGPRs, issued here and needed after the
    // transform.  Starts: blocks kA .. kA + 2 VB - 1; ends: kA + Mh .. kA + Mh + 2 VB; and the end of the span of
    // samples that enters this pair's transforms (error bound).
    double sb[2 * FFT_VB], eb[2 * FFT_VB + 1];
    double sb1[CC ? 2 * FFT_VB : 1], eb1[CC ? 2 * FFT_VB + 1 : 1];
    double span_end, span_start1, span_end1;                     // (sums of the samples over the span: its centred energy)
    const int n_seg = (M + FFT_SEG - 1) / FFT_SEG;
    if (kA + n_seg + 2 * FFT_VB <= a.nb) {                       // away from the end of the stream: consecutive entries, wide loads
#pragma unroll
        for (int c = 0; c < 2 * FFT_VB; ++c) sb[c] = a.ubase[kA + c];
#pragma unroll
        for (int c = 0; c < 2 * FFT_VB + 1; ++c) eb[c] = a.ubase[kA + Mh + c];
        span_end = a.ubase[kA + n_seg + 2 * FFT_VB];
        span_start1 = a.sbase[kA];
        span_end1 = a.sbase[kA + n_seg + 2 * FFT_VB];
        if (CC) {
#pragma unroll
            for (int c = 0; c < 2 * FFT_VB; ++c) sb1[c] = a.sbase[kA + c];
#pragma unroll
            for (int c = 0; c < 2 * FFT_VB + 1; ++c) eb1[c] = a.sbase[kA + Mh + c];
        }
    } else {
#pragma unroll
        for (int c = 0; c < 2 * FFT_VB; ++c) {
            int64_t bi = kA + c;
            bi = bi < a.nb ? bi : a.nb;
            sb[c] = a.ubase[bi];
            if (CC) sb1[c] = a.sbase[bi];
        }
#pragma unroll
        for (int c = 0; c < 2 * FFT_VB + 1; ++c) {
            int64_t bi = kA + Mh + c;
            bi = bi < a.nb ? bi : a.nb;
            eb[c] = a.ubase[bi];
            if (CC) eb1[c] = a.sbase[bi];
        }
        int64_t bi = kA + n_seg + 2 * FFT_VB;
        bi = bi < a.nb ? bi : a.nb;
        span_end = a.ubase[bi];
        span_end1 = a.sbase[bi];
        int64_t b0 = kA < a.nb ? kA : a.nb;
        span_start1 = a.sbase[b0];
    }
    cpx v[sushi_fft::PER];
    sushi_fft::fft_wave_mfma<1>(yl, v, tid, lds, tw, mb);
    // keep the window loads below the last pass: hoisted above it (the scheduler's preference) they do not
    // fit the register budget next to the radix-16 butterflies and get spilled to scratch one by one.
    // `after_fft` is an opaque zero that the asm "computes" from the needed outputs; added to the load
    // offsets it makes the loads depend on the finished transform.
    // (an asm statement takes at most 30 operands: the outputs are chained through in groups of 4)
#pragma unroll
    for (int g = 0; g < HPT; g += 4) {
        asm volatile("v_mov_b32 %0, 0"
                     : "=v"(after_fft)
                     : "v"(v[g + 0].x), "v"(v[g + 0].y), "v"(v[g + 1].x), "v"(v[g + 1].y), "v"(v[g + 2].x), "v"(v[g + 2].y),
                       "v"(v[g + 3].x), "v"(v[g + 3].y), "v"(after_fft));
    }
    // wave-uniform floats made from float64 arithmetic live in VGPRs unless told otherwise: pin them to SGPRs
    auto uniform = [](const float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); };
    // window energy = ub0[h][b] (+ dub[h][b] if the window's end falls one block further) + (urel[q + M] - urel[q])
    float ub0[2][FFT_VB], dub[2][FFT_VB];
    float us0[CC ? 2 : 1][FFT_VB], dus[CC ? 2 : 1][FFT_VB];      // (METHOD 1) the same for the window sums
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int b = 0; b < FFT_VB; ++b) {
            const float e0 = (float)(eb[h * FFT_VB + b] - sb[h * FFT_VB + b]);       // window end's base - start's
            const float e1 = (float)(eb[h * FFT_VB + b + 1] - sb[h * FFT_VB + b]);
            ub0[h][b] = uniform(e0);
            dub[h][b] = uniform(e1 - e0);
            if (CC) {
                const float f0 = (float)(eb1[h * FFT_VB + b] - sb1[h * FFT_VB + b]);
                const float f1 = (float)(eb1[h * FFT_VB + b + 1] - sb1[h * FFT_VB + b]);
                us0[h][b] = uniform(f0);
                dus[h][b] = uniform(f1 - f0);
            }
        }
    }
    const float zn = uniform((float)sqrt(fmax(span_end - sb[0], 0.0)));
    zn_out = zn;
    {
        // energy of the CENTRED samples that enter this pair's transforms (what the f32 error of the cross term scales with)
        const int64_t s_lo = qbase < n ? qbase : n;
        const int64_t s_hi64 = (kA + n_seg + 2 * FFT_VB) * (int64_t)FFT_SEG;
        const int64_t s_hi = s_hi64 < n ? s_hi64 : n;
        const double c = a.dst_stats[1];
        const double e2 = (span_end - sb[0]) - 2.0 * c * (span_end1 - span_start1) + c * c * (double)(s_hi - s_lo);
        znc_out = uniform((float)sqrt(fmax(e2, 0.0)) * 1.0000005f);
    }
    // sum T I = y' / scale + c sum T  (block spectra of the centred stream, pattern spectra scaled: module header)
    const float tU = uniform((float)(tc.tU - 2.0 * (double)tc.c_sum_t));
    const float m2s = uniform(-2.0f * tc.inv_scale);
    const float inv_s = uniform(tc.inv_scale);
    const float inv_tnorm = uniform(CC ? tc.inv_tnorm_c : tc.inv_tnorm);
    const float neg_inv_m = uniform(-tc.inv_m);
    // (METHOD 1) a window variance sum below this is inside its own rounding error: four times the modelled error
    const float tau = uniform(4.0f * 5.9604645e-8f * zn * zn * ccoeff_cd(sqrtf(tc.inv_m)));

    // ---- f32 scores (ranking only: the near-minimum ones are re-evaluated exactly) ----
    // METHOD 0: score = num / (sqrt(wU) * tnorm), and 1 where wU <= 0 (cv2's `t = 0` case: the test
    // diff2 <= min(0.5, 10*eps*wU) can only hold for wU <= 0).  cv2's clamp score <= 1 is applied here too:
    // it creates exact ties at 1.0 (no-match windows), and ties must all become candidates for the lowest
    // index to win.
    const int carry_from = FFT_SEG - Ml - tid;                   // window end one block further iff FT*(r % RPB) >= this
    float best_s = __builtin_inff();
    float max_rs = 0.f;
    int any_unc = 0;
    auto score_all = [&](auto interior_tag) {
        constexpr bool INTERIOR = decltype(interior_tag)::value;
        load_group(0, ra, rb, sa, sb_, interior_tag);
#pragma unroll
        for (int g = 0; g < NG; ++g) {                      // (ties are settled by position afterwards)
            if (g + 1 < NG) load_group(g + 1, ra_n, rb_n, sa_n, sb_n, interior_tag);
#pragma unroll
            for (int q = 0; q < GQM; ++q) {
                const int r = g * (GQM / 2) + q / 2;
                const int half = q & 1;
                const int blk = r / RPB;
                const int pos = tid + FT * r + half * FH;
                const bool carry = FT * (r % RPB) >= carry_from;
                const float wU = (ub0[half][blk] + (carry ? dub[half][blk] : 0.f)) + (rb[q] - ra[q]);   // sum I^2
                const float yv = half ? v[r].y : v[r].x;
                float score, rs;
                bool certain;
                if (CC) {
                    const float wS = (us0[half][blk] + (carry ? dus[half][blk] : 0.f)) + (sb_[q] - sa[q]);   // sum I
                    const float num = yv * inv_s;                                    // sum (T - mean T) I: the spectra are of the centred pattern
                    const float d2 = __builtin_fmaf(wS * neg_inv_m, wS, wU);         // sum I^2 - (sum I)^2 / M
                    certain = d2 > tau;
                    rs = __builtin_amdgcn_rsqf(d2);
                    const float cc = __builtin_amdgcn_fmed3f(num * rs * inv_tnorm, -1.0f, 1.0f);
                    score = certain ? 1.0f - cc : UNCERTAIN;
                } else {
                    const float num = __builtin_fmaf(yv, m2s, tU + wU);              // sum (T - I)^2 = sum T^2 + sum I^2 - 2 sum T I
                    // a window without energy scores 1 (cv2's t = 0 case): clamped to a tiny energy its score is huge before
                    // the clamp to 1, and its 1/|window| blows the pair's bound up so that every position of the pair goes to
                    // the exact stages -- right, and one v_max instead of a compare and two selects per position (a pattern
                    // without energy, where num can be 0 as well, is handled before the loop)
                    rs = __builtin_amdgcn_rsqf(fmaxf(wU, 1e-30f));
                    score = num * rs * inv_tnorm;                                    // ~1 ulp: this stage only ranks
                    score = __builtin_amdgcn_fmed3f(score, 0.0f, 1.0f);              // both clamps (keys need score >= 0)
                    certain = true;
                }
                bool valid = true;
                if (!INTERIOR) {
                    valid = pos >= plo && pos < phi;
                    score = valid ? score : __builtin_inff();
                }
                ps.scores[half * HPT + r] = score;
                if (CC) {
                    best_s = fminf(best_s, score >= 0.f ? score : __builtin_inff());
                    any_unc |= (valid && !certain) ? 1 : 0;
                } else {
                    best_s = fminf(best_s, score);
                }
                max_rs = fmaxf(max_rs, (certain && valid) ? rs : 0.f);
            }
            if (g + 1 < NG) {
#pragma unroll
                for (int q = 0; q < GQM; ++q) {
                    ra[q] = ra_n[q]; rb[q] = rb_n[q];
                    if (CC) { sa[q] = sa_n[q]; sb_[q] = sb_n[q]; }
                }
            }
        }
    };
    if (interior) score_all(std::true_type()); else score_all(std::false_type());
    if (!CC && !(tc.tU > 0.0)) {
        // a pattern of zeros: cv2's result is all ones (t = 0 everywhere), while num * rs * (1 / 0) above is NaN where the window
        // has no energy either
#pragma unroll
        for (int q = 0; q < 2 * HPT; ++q) ps.scores[q] = ps.scores[q] < __builtin_inff() || ps.scores[q] != ps.scores[q] ? 1.0f : ps.scores[q];
        best_s = 1.0f;
        max_rs = fmaxf(max_rs, 1e15f);
    }
    ps.best = best_s;
    ps.max_rs = max_rs;
    ps.any_uncertain = any_unc;
}

// error bound of a pair in score units (module header, sushi_common.hpp FFT_KE).
// METHOD 0: the cross term's 2 * KE * eps * |Z| / |window| plus the window energy's own f32 rounding,
//           16 * eps * |Z|^2 / (|T| * |window|)
// METHOD 1: numerator error / (|T_c| |W_c|) + the relative error of 1 / sqrt(variance sum) (the score is <= 1 in size)
template <int METHOD>
__device__ __forceinline__ float pair_error_model(float zn, float zn_c, float max_rs, const TemplConsts& tc, float q2,
                                                  float inv_scale, int mac_passes) {
    const float eps = 5.9604645e-8f;                             // 2^-24
    // quantisation of the Y row: every stored half is off by <= 2^-11 of its size (round to nearest), independently; the
    // inverse transform sums N of them: variance (2^-22 / 3) * sum |Y(f)|^2 (+ the subnormal floor), Y_KQ deviations
    // (2^-22 / 3) x (the row's own rounding, once per accumulating pass of mac_long_kernel: a pattern of more than MAC_SMAX_LONG
    // segments re-rounds the partial row every pass; + its two factors' roundings: module header)
    const float sigma_y = sqrtf(q2 * (7.9472862e-8f * (float)(2 + mac_passes)) + (float)FN * 1.2e-15f) * inv_scale;
    if (METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED) {
        const float ism = sqrtf(tc.inv_m);
        const float z = fmaxf(zn, zn_c);
        // (numerator: the cross term of the CENTRED pattern, FFT_KE eps |T_c| |Z|, over |T_c| |W_c|)
        return eps * max_rs * z * (FFT_KE + ccoeff_cd(ism) * z * max_rs) + Y_KQ * sigma_y * max_rs * tc.inv_tnorm_c;
    }
    return eps * max_rs * (2.0f * FFT_KE * zn_c + 16.0f * zn * zn * tc.inv_tnorm) + 2.0f * Y_KQ * sigma_y * max_rs * tc.inv_tnorm;
}

// sum over the workgroup of a per-thread value, the same in ifft_kernel and collect_kernel whatever the order the waves
// arrive in: 16 x the largest wave sum (an upper bound, and waves hold similar shares of a row's energy)
// Wave reductions on the VALU's cross-lane paths (DPP inside rows of 16 lanes, four readlanes across the rows): __shfl_*
// goes through ds_bpermute_b32 and needs an address register per step, which ifft_kernel does not have to spare.
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
template <class Op>
__device__ __forceinline__ float row_reduce_f32(float v, Op op) {          // every lane ends with its row's result
    v = op(v, dpp_f32<0xB1>(v));                                 // quad_perm [1,0,3,2]
    v = op(v, dpp_f32<0x4E>(v));                                 // quad_perm [2,3,0,1]
    v = op(v, dpp_f32<0x141>(v));                                // row_half_mirror
    v = op(v, dpp_f32<0x140>(v));                                // row_mirror
    return v;
}
template <class Op>
__device__ __forceinline__ float wave_reduce_f32(float v, Op op) {         // wave-uniform result
    v = row_reduce_f32(v, op);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return op(op(r0, r1), op(r2, r3));
}
__device__ __forceinline__ float wave_sum_f32(float v) { return wave_reduce_f32(v, [](float a, float b) { return a + b; }); }
__device__ __forceinline__ float wave_min_f32(float v) { return wave_reduce_f32(v, [](float a, float b) { return fminf(a, b); }); }
__device__ __forceinline__ float wave_max_f32(float v) { return wave_reduce_f32(v, [](float a, float b) { return fmaxf(a, b); }); }
// (bit patterns of floats >= 0: the integer order is the float order, and nothing is dropped for being a NaN)
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    return __float_as_uint(wave_reduce_f32(__uint_as_float(v), [](float a, float b) { return __uint_as_float(__float_as_uint(a) > __float_as_uint(b) ? __float_as_uint(a) : __float_as_uint(b)); }));
}

// shared state of one pair's epilogue (ifft_kernel)
struct IfftShared {
    unsigned red_min, red_rs;        // float bits (both >= 0: unsigned order == float order)
    float red_q[FT / 64];            // per wave: energy of its share of the Y row
    int ccnt, unc_any;
};

template <int METHOD>
__device__ __forceinline__ void ifft_one(const IfftArgs& a, const int slot, float* lds, IfftShared& sh, const int tid) {
    unsigned& red_min = sh.red_min; unsigned& red_rs = sh.red_rs; float (&red_q)[FT / 64] = sh.red_q; int& ccnt = sh.ccnt; int& unc_any = sh.unc_any;
    // which pair: by default the workgroup index; with a schedule the pairs that read the same region of the
    // destination stream run back to back on one XCD, so that the prefix-sum lines they share are fetched into that
    // XCD's L2 once instead of once per search
    const int pr = a.order ? a.order[slot] : slot;
    sushi_fft::uint4v yl[4];
    const float q2 = load_y(yl, a.y + (size_t)pr * (FN / 2), tid);     // in flight while the descriptors below arrive
    const sushi_fft::MfmaB mb = dft16_operands(tid);
    const sushi_fft::WTwiddles tw = sushi_fft::load_wtwiddles<1>(tid, twiddles());
    const int lane = tid & 63;
    {
        const float qw = wave_sum_f32(q2);
        if (lane == 0) red_q[tid >> 6] = qw;                           // read after the barriers inside the transform
    }
    const int k = __builtin_amdgcn_readfirstlane(a.pairmap[pr]);       // wave-uniform: everything derived from it is scalar
    const SearchDesc sd = a.searches[k];
    const int i = pair_of_search(a.sub_first_pair, pr, sd);
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const TemplConsts tc = a.tconst[k];
    // the pair's row of the candidate array starts as all NO_KEY (memset at the start of the run): only what exists is written
    unsigned long long* __restrict__ cout = a.cand + (size_t)pr * FFT_ROW;
    if (METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED && tc.flat) {
        // a pattern without variance: cv2's result is all ones (refine_kernel answers position 0); nothing to rank
        if (tid == 0) { cout[FFT_CAND + 1] = 0ull; a.pair_lb[pr] = __builtin_inff(); }
        return;
    }
    if (tid == 0) { ccnt = 0; unc_any = 0; red_min = 0x7f800000u; red_rs = 0u; }   // read after the barriers inside the transform
    PairScores ps;
    int plo, phi;
    float zn, zn_c;
    score_pair<METHOD>(a, yl, mb, sd, tc, lay.pair0 + i, lds, tid, tw, ps, plo, phi, zn, zn_c);
    // minimum of the pair and the largest 1/|window| (error bound): 32-bit wave reductions, then one LDS atomic each per
    // wave and ONE barrier -- the workgroup's tail is serial time on a CU that holds two workgroups
    const float wmin = wave_min_f32(ps.best), wrs = wave_max_f32(ps.max_rs);
    if (lane == 0) {
        atomicMin(&red_min, __float_as_uint(wmin));                    // scores are >= 0 or +inf
        atomicMax(&red_rs, __float_as_uint(wrs));
    }
    if (METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED && __ballot(ps.any_uncertain) != 0ull && lane == 0) unc_any = 1;
    __syncthreads();
    const float lmin_s = __uint_as_float(red_min), rs_max = __uint_as_float(red_rs);
    const bool have_min = lmin_s < __builtin_inff();
    static_assert(FT / 64 == 16, "one row of lanes reads the sixteen wave sums");
    const float qmax = row_reduce_f32(red_q[lane & 15], [](float a, float b) { return fmaxf(a, b); });
    const int mac_passes = (lay.n_seg + MAC_SMAX_LONG - 1) / MAC_SMAX_LONG;
    const float e_model = pair_error_model<METHOD>(zn, zn_c, rs_max, tc, (float)(FT / 64) * qmax, tc.inv_scale, mac_passes);
    const float e_pair = fmaxf(0.5f * a.delta, e_model);
    // positions leave this kernel relative to the search's window: p = (pair's first sample + pos) - win_start
    const int64_t shift = (lay.pair0 + i) * (int64_t)FFT_STEP * FFT_SEG - sd.win_start;
    if (tid == 0) {
        cout[FFT_CAND + 1] = ((unsigned long long)__float_as_uint(e_model) << 32) | __float_as_uint(e_pair);
        // the smallest lower bound among the pair's positions: refine_kernel reads this one float per pair and opens the row
        // only of pairs that can hold the search's extremum (it used to read every row of every pair: 10 KB per search)
        const bool unc = METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED && unc_any;
        a.pair_lb[pr] = unc ? 0.f : (have_min ? fmaxf(lmin_s - e_pair, 0.f) : __builtin_inff());
        if (a.slb && have_min && !unc) {
            // The pair's lower bound (slb_kernel) must not be above any of its exact scores, and the exact score of its best position
            // is at most lmin_s + e_pair.  Checked on every pair that IS transformed -- among them, per run, one pair per audited
            // search that the bound had excluded (survivor_kernel): where it fails the search is evaluated at every position.
            // (TM_SQDIFF_NORMED scores are clamped at 1, cv2's rule, the bound is not: a pair far louder than the pattern has
            // a bound in the thousands and every score 1)
            const float s = METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED ? a.slb[pr] : fminf(a.slb[pr], 1.0f), ub = lmin_s + e_pair;
            const unsigned char am = a.audit_mark ? a.audit_mark[pr] : (unsigned char)0;
            const bool audit = (am & MARK_AUDITED) != 0;
            if (s > ub * 1.00001f + 1e-7f) {
                a.viol[a.first_search + k] = 1;
                atomicAdd(&a.counters->slb_violations, 1);
            }
            if (audit) {
                atomicAdd(&a.counters->excluded_audited, 1ull);
                if (am & MARK_SECOND_LOOK) atomicAdd(&a.counters->second_look_audited, 1ull);
                const float ratio = s > 0.f ? s / fmaxf(ub, 1e-30f) : 0.f;
                if (__float_as_uint(ratio) > *(volatile uint32_t*)&a.counters->max_slb_ratio_bits)
                    atomicMax(&a.counters->max_slb_ratio_bits, __float_as_uint(ratio));
            }
        }
    }
    // a position can be the search's minimum only if score - e <= (smallest score + e) of the search; inside the
    // pair that is score <= lmin_s + 2 e (refine_kernel applies the search-wide threshold to the stored lower bounds);
    // uncertain positions (METHOD 1) always can
    const float thr = lmin_s + 2.0f * e_pair;
    const bool mine = METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED ? ((ps.best <= thr && have_min) || ps.any_uncertain)
                                                               : (ps.best <= thr && have_min);
    if (mine) {                                                 // few lanes (often one wave) get past this
        // slots 0 .. FFT_CAND-1: candidates, written where they are found; whoever draws slot FFT_CAND writes the marker
        // "more candidate positions than slots" (a lower bound of everything unlisted, position 0xffffffff): refine_kernel
        // flags the search if that bound is under the search's threshold
        const float unlisted_lb = (METHOD == SUSHI_HIP_METHOD_CCOEFF_NORMED && unc_any) ? 0.f : fmaxf(lmin_s - e_pair, 0.f);
        int lowest = 0x7fffffff;                                // lowest position of this thread that holds the minimum
#pragma unroll
        for (int q = 0; q < 2 * HPT; ++q) {
            const float sc = ps.scores[q];
            if (sc <= thr && sc < __builtin_inff()) {
                const int pos = tid + FT * (q % HPT) + (q / HPT) * FH;
                if (sc == lmin_s) lowest = pos < lowest ? pos : lowest;
                const int slot = atomicAdd(&ccnt, 1);
                if (slot < FFT_CAND) cout[slot] = make_key(fmaxf(sc - e_pair, 0.f), (unsigned)((int64_t)pos + shift));
                else if (slot == FFT_CAND) cout[FFT_CAND] = make_key(unlisted_lb, 0xffffffffu);
            }
        }
        // the pair's upper bound (its smallest score + e) at the lowest position holding it: ties inside a pair are rare, and
        // atomicMin over the keys settles them by position
        if (lowest != 0x7fffffff)
            atomicMin(a.gkeys + a.first_search + k, make_key(lmin_s + e_pair, (unsigned)((int64_t)lowest + shift)));
    }
    // the pair's audit runs: AUDIT_RUNS x FFT_AUDIT consecutive positions at a pseudo-random place (a hash of the pair index)
    // leave with their plain f32 scores whether or not they are candidates; refine_kernel evaluates AUDIT_RUNS runs per search
    // exactly, from as many different transformed pairs as there are (consecutive positions: their windows are one another's but
    // for a few samples, so a run costs the loads of ONE position)
    {
        constexpr int RUNP = AUDIT_RUNS * FFT_AUDIT;                     // FT % RUNP == 0: one r, one half for the whole stretch
        const unsigned h = ((unsigned)(a.sub_first_pair + pr) * 2654435761u) >> 7;
        const int pos_a = RUNP * (int)(h % (unsigned)(2 * FH / RUNP));
        const int j = tid - pos_a % FT;
        if (j >= 0 && j < RUNP) {
            const int qa = (pos_a / FH) * HPT + (pos_a % FH) / FT;
            float sc = __builtin_inff();
#pragma unroll
            for (int q = 0; q < 2 * HPT; ++q) sc = q == qa ? ps.scores[q] : sc;
            if (sc >= 0.f && sc < __builtin_inff()) cout[FFT_CAND + 2 + j] = make_key(sc, (unsigned)((int64_t)(pos_a + j) + shift));
        }
    }
}

// One workgroup per pair; with `count` (a list whose length only the device knows: the pairs the bound left) a FIXED grid strides
// over the list instead of one workgroup per possible entry -- 346,000 workgroups that found their slot empty were 0.3 ms of a step.
template <int METHOD>
__global__ __launch_bounds__(FT, 8)
void ifft_kernel(IfftArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    __shared__ IfftShared sh;
    if (a.count && (int)blockIdx.x >= *a.count) return;               // a list shorter than the grid
    ifft_one<METHOD>(a, (int)blockIdx.x, lds, sh, (int)threadIdx.x);
}
template <int METHOD>
__global__ __launch_bounds__(FT, 8)
void ifft_list_kernel(IfftArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    __shared__ IfftShared sh;
    const int n = *a.count;
    for (int slot = a.list_first + blockIdx.x; slot < n; slot += gridDim.x) {
        // (everything an iteration needs is loaded inside it, off a thread index the compiler cannot see through: left to hoist
        // the transform's per-thread constants out of the loop it spills them -- collect_kernel's lesson)
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        ifft_one<METHOD>(a, slot, lds, sh, tid);
        __syncthreads();                                               // the shared state is consumed before the next pair resets it
    }
}
