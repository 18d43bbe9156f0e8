// sushi_amd/csrc/sushi_fft_threshold.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// the threshold run's own kernels (sushi_hip_batch_run_threshold, DESIGN.md 3.10).  The pair exclusion is the argmin run's, with
// the search's running threshold U replaced by the caller's threshold in ranking units (sushi_fft.hip ranking_key); the exact
// evaluation of the listed pairs is sushi_curve.hip's threshold_tiles_kernel.  The rules it shares with the other runs are
// sushi_fft_bound.inc's (bound_excludes, is_audit_pair, append_pairs); what it shares with the best-K run alone is here:
// PairRunArgs, the head of both runs' kernel arguments, and audit_pair, the audit of one evaluated pair.  Per sub-batch:
//   thr_seed_kernel     U of every search (gkeys) and no pilot pair (plist = -1): survivor_kernel / survivor2_kernel exclude a pair
//                       only if its lower bound is above U -- no exact score of the pair can pass
//   (bound, survivors, second look: unchanged)           threshold_tiles_kernel pass 0 over the listed pairs
//   thr_check_kernel    the bound held to what every listed pair really scores; an audited excluded pair with a hit, or with a
//                       score below its bound, marks its search violated
//   thr_extend_kernel   the pairs of violated searches that were not listed: listed now (threshold_tiles_kernel pass 0 again)
//   thr_scan_kernel     per search, in pair order: each evaluated pair's first output slot, the search's hit count
//                       (threshold_tiles_kernel pass 1 then writes the hits)

__global__ __launch_bounds__(256)
void thr_seed_kernel(unsigned long long* __restrict__ gkeys, int n_sub, unsigned long long key, int* __restrict__ plist) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n_sub) { gkeys[k] = key; plist[k] = -1; }
}

// What the kernels of both listed-pair runs (here and in sushi_fft_best.inc) read of their sub-batch (sushi_fft.hip pair_run_args).
struct PairRunArgs {
    const SearchDesc* searches;       // the sub-batch's searches
    int first_search;
    int sub_first_pair;
    int n_sub;
    int n_pairs;
    const int* pairmap;
    const uint32_t* rows;             // [pairs][THR_SLOT_WORDS] (the tile kernels' output)
    const float* slb;
    unsigned char* audit_mark;        // MARK_* bits (sushi_internal.hpp): MARK_AUDITED, MARK_LISTED (= evaluated); the run kinds' own bits: their kernels
    int* viol;                        // [all searches]
    RunCounters* counters;
    int method;
};

// The audit of one evaluated pair (ifft_kernel's, with the pair's exact scores instead of its f32 ones): its bound against `ub`, the
// smallest ranking score of its tiles.  A bound above it -- or `also(ub)`, the run kind's own further reason -- marks the search
// violated (returned); `audited` (the bound had excluded the pair) counts it and records the ratio.
template <class Also>
__device__ __forceinline__ bool audit_pair(const PairRunArgs& a, const int pr, const bool audited, Also&& also) {
    const uint32_t* __restrict__ row = a.rows + (size_t)pr * THR_SLOT_WORDS;
    float ub = __builtin_inff();
    for (int t = 0; t < TILES_PER_PAIR; ++t) ub = fminf(ub, __uint_as_float(row[THR_MIN + t]));
    // (TM_SQDIFF_NORMED scores are clamped at 1, cv2's rule, the bound is not)
    const float s = a.method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? a.slb[pr] : fminf(a.slb[pr], 1.0f);
    const bool violated = s > ub * 1.00001f + 1e-7f || also(ub);
    if (violated) {
        a.viol[a.first_search + a.pairmap[pr]] = 1;
        atomicAdd(&a.counters->slb_violations, 1);
    }
    if (audited) {
        atomicAdd(&a.counters->excluded_audited, 1ull);
        const float ratio = s > 0.f ? s / fmaxf(ub, 1e-30f) : 0.f;
        atomicMax(&a.counters->max_slb_ratio_bits, __float_as_uint(ratio));
    }
    return violated;
}

struct ThrArgs : PairRunArgs {        // (audit_mark NULL: every pair is evaluated)
    uint32_t* rows_w;
    const int* list; const int* list_count;
    int* list3; int* list3_count;     // thr_extend_kernel: the pairs of violated searches that were not listed
    int64_t* counts_out;              // [all searches]
};

// one thread per listed pair
__global__ __launch_bounds__(256)
void thr_check_kernel(ThrArgs a) {
    const int n = *a.list_count;
    for (int slot = blockIdx.x * 256 + threadIdx.x; slot < n; slot += gridDim.x * 256) {
        const int pr = a.list[slot];
        const bool audit = (a.audit_mark[pr] & MARK_AUDITED) != 0;
        // an audited pair was excluded: a hit in it is a violation whatever its margin
        audit_pair(a, pr, audit, [&](float) {
            if (!audit) return false;
            const uint32_t* __restrict__ row = a.rows + (size_t)pr * THR_SLOT_WORDS;
            int hits = 0;
            for (int t = 0; t < TILES_PER_PAIR; ++t) hits += (int)row[THR_COUNT + t];
            return hits > 0;
        });
    }
}

// every pair of a violated search that was not listed is listed now (list3), and marked evaluated
__global__ __launch_bounds__(256)
void thr_extend_kernel(ThrArgs a) {
    const int pr = blockIdx.x * 256 + threadIdx.x;
    bool add = false;
    if (pr < a.n_pairs && a.viol[a.first_search + a.pairmap[pr]] && !(a.audit_mark[pr] & MARK_LISTED)) {
        add = true;
        a.audit_mark[pr] |= MARK_LISTED;
    }
    append_pairs(a.list3, a.list3_count, a.counters, add, pr);
}

// one workgroup per search: an exclusive scan of its evaluated pairs' hit counts in pair order (= position order)
__global__ __launch_bounds__(256)
void thr_scan_kernel(ThrArgs a) {
    __shared__ int wsum[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchDesc sd = a.searches[k];
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const int p0 = first_pair_in_sub(a.sub_first_pair, sd);
    int running = 0;
    for (int base = 0; base < lay.n_pairs; base += 256) {
        const int i = base + tid;
        const int pr = p0 + i;
        const bool evaluated = i < lay.n_pairs && (!a.audit_mark || (a.audit_mark[pr] & MARK_LISTED));
        int c = 0;
        if (evaluated) {
            const uint32_t* __restrict__ row = a.rows + (size_t)pr * THR_SLOT_WORDS;
            for (int t = 0; t < TILES_PER_PAIR; ++t) c += (int)row[THR_COUNT + t];
        }
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int before = running;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        if (evaluated) a.rows_w[(size_t)pr * THR_SLOT_WORDS + THR_OFF] = (uint32_t)(before + incl - c);
        running += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) a.counts_out[a.first_search + k] = running;
}
