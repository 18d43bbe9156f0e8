// sushi_amd/csrc/sushi_fft_threshold.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// the threshold run's own kernels (sushi_hip_batch_run_threshold, DESIGN.md 3.10).  The pair exclusion is the argmin run's, with
// the search's running threshold U replaced by the caller's threshold in ranking units; the exact evaluation of the listed pairs is
// sushi_curve.hip's threshold_tiles_kernel.  Per sub-batch:
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

struct ThrArgs {
    const SearchDesc* searches;       // the sub-batch's searches
    int first_search;
    int sub_first_pair;
    int n_sub;
    int n_pairs;
    const int* pairmap;
    const uint32_t* rows;             // [pairs][THR_SLOT_WORDS] (threshold_tiles_kernel's output)
    uint32_t* rows_w;
    const float* slb;
    unsigned char* audit_mark;        // bit 0 audited (excluded all the same), bit 1 listed; NULL: every pair is evaluated
    const int* list; const int* list_count;
    int* list3; int* list3_count;     // thr_extend_kernel: the pairs of violated searches that were not listed
    int* viol;                        // [all searches]
    RunCounters* counters;
    int method;
    int64_t* counts_out;              // [all searches]
};

// one thread per listed pair (ifft_kernel's audit, with the pair's exact scores instead of its f32 ones)
__global__ __launch_bounds__(256)
void thr_check_kernel(ThrArgs a) {
    const int n = *a.list_count;
    for (int slot = blockIdx.x * 256 + threadIdx.x; slot < n; slot += gridDim.x * 256) {
        const int pr = a.list[slot];
        const uint32_t* __restrict__ row = a.rows + (size_t)pr * THR_SLOT_WORDS;
        int hits = 0;
        float ub = __builtin_inff();
        for (int t = 0; t < TILES_PER_PAIR; ++t) { hits += (int)row[THR_COUNT + t]; ub = fminf(ub, __uint_as_float(row[THR_MIN + t])); }
        // (TM_SQDIFF_NORMED scores are clamped at 1, cv2's rule, the bound is not)
        const float s = a.method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? a.slb[pr] : fminf(a.slb[pr], 1.0f);
        const bool audit = (a.audit_mark[pr] & 1) != 0;
        // an audited pair was excluded: a hit in it is a violation whatever its margin
        if (s > ub * 1.00001f + 1e-7f || (audit && hits > 0)) {
            a.viol[a.first_search + a.pairmap[pr]] = 1;
            atomicAdd(&a.counters->slb_violations, 1);
        }
        if (audit) {
            atomicAdd(&a.counters->excluded_audited, 1ull);
            const float ratio = s > 0.f ? s / fmaxf(ub, 1e-30f) : 0.f;
            atomicMax(&a.counters->max_slb_ratio_bits, __float_as_uint(ratio));
        }
    }
}

// every pair of a violated search that was not listed is listed now (list3), and marked evaluated
__global__ __launch_bounds__(256)
void thr_extend_kernel(ThrArgs a) {
    const int pr = blockIdx.x * 256 + threadIdx.x;
    bool add = false;
    if (pr < a.n_pairs && a.viol[a.first_search + a.pairmap[pr]] && !(a.audit_mark[pr] & 2)) {
        add = true;
        a.audit_mark[pr] |= 2;
    }
    const unsigned long long m = __ballot(add);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && m) {
        base = atomicAdd(a.list3_count, __popcll(m));
        atomicAdd(&a.counters->pairs_transformed, (unsigned long long)__popcll(m));
    }
    base = __shfl(base, 0, 64);
    if (add) a.list3[base + __popcll(m & ((1ull << lane) - 1ull))] = pr;
}

// one workgroup per search: an exclusive scan of its evaluated pairs' hit counts in pair order (= position order)
__global__ __launch_bounds__(256)
void thr_scan_kernel(ThrArgs a) {
    __shared__ int wsum[4];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const SearchDesc sd = a.searches[k];
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const int p0 = sd.first_pair - a.sub_first_pair;
    int running = 0;
    for (int base = 0; base < lay.n_pairs; base += 256) {
        const int i = base + tid;
        const int pr = p0 + i;
        const bool evaluated = i < lay.n_pairs && (!a.audit_mark || (a.audit_mark[pr] & 2));
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
