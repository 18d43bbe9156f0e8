// sushi_amd/csrc/sushi_fft_best.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// the best-K run's own kernels (sushi_hip_batch_run_best, DESIGN.md 3.11).  The pair exclusion is the argmin run's, with the
// search's running threshold U FOUND by the run itself: the ranking score of the K-th pick that greedy suppression makes from the
// pairs evaluated so far (best_select_kernel, sushi_curve.hip, leaves it in gkeys).  A pair is listed for exact evaluation
// (best_tiles_kernel) as soon as its bound does not exclude it under the U of the moment, and a pair once evaluated stays so:
// audit_mark bit 1.  Per sub-batch, a fixed launch sequence, every list length a count on the device:
//   best_seed_kernel      per search: its BEST_SEED_EXTRA + K pairs of smallest bound are evaluated first
//   best_survivor_kernel  a round of escalation: the pairs not yet evaluated that their search's U does not exclude
//                         (band-split form: then the second look, survivor2_kernel)
//   best_final_kernel     after the last round: a search that would still list a pair is unsettled (every pair of it is evaluated);
//                         of the others, the audit's hashed excluded pair is evaluated all the same
//   best_check_kernel     the bound held to what every audited pair really scores
//   best_extend_kernel    every pair not yet evaluated of the unsettled and the violated searches
// A search is selected again (best_select_kernel) after every round that evaluated a pair of it: `stamp` in its flags word.

constexpr int BEST_SEED_EXTRA = 2;     // pairs seeded beyond K: K picks S apart lie in at most K pairs; two more for picks next to a pair's ends
constexpr int BEST_ROUNDS = 2;         // escalation rounds before the last one, which settles whatever is left

struct BestArgs {
    const SearchDesc* searches;       // the sub-batch's searches
    int first_search;
    int sub_first_pair;
    int n_sub;
    int n_pairs;
    int k;
    const int* pairmap;
    const int* order;                 // the L2-friendly schedule of all pairs (lists keep its order)
    const uint32_t* rows;             // [pairs][THR_SLOT_WORDS] (best_tiles_kernel's output)
    const float* slb;
    unsigned char* audit_mark;        // bit 0 audited (excluded all the same), bit 1 evaluated, bit 2 by the second look, bit 3 by best_final_kernel
    unsigned long long* gkeys;        // [all searches]
    unsigned long long tkey;          // the threshold as a search key, NO_KEY: none
    int* list; int* list_count;
    int* flags;                       // [all searches] the stamp of the last round that evaluated a pair of the search
    int stamp;
    int* need;                        // [all searches] 1: unsettled after the last round
    int* viol;                        // [all searches]
    RunCounters* counters;
    int method;
    unsigned audit_seq; int audit_every;
};

// survivor_kernel's rule: a pair is excluded only if its bound, with the slack, is above U; a search whose U is 1 ties everywhere
__device__ __forceinline__ bool best_excluded(const BestArgs& a, const int pr, const int k) {
    const unsigned long long g = a.gkeys[a.first_search + k];
    const float U = g == NO_KEY ? __builtin_inff() : key_score(g);
    return U < 0.9999f && a.slb[pr] > U * 1.000001f + 1e-7f;
}

// `add` pairs of this wave to the list, in lane order
__device__ __forceinline__ void best_append(const BestArgs& a, const bool add, const int pr) {
    const unsigned long long m = __ballot(add);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && m) {
        base = atomicAdd(a.list_count, __popcll(m));
        atomicAdd(&a.counters->pairs_transformed, (unsigned long long)__popcll(m));
    }
    base = __shfl(base, 0, 64);
    if (add) a.list[base + __popcll(m & ((1ull << lane) - 1ull))] = pr;
}

// one workgroup per search: no pair evaluated yet, U = the threshold's (or none); then the pairs of smallest bound are listed, one
// per round in (bound, pair) order -- "no bound" (-inf) first --, except those the threshold already excludes
__global__ __launch_bounds__(256)
void best_seed_kernel(BestArgs a) {
    __shared__ unsigned long long red[4];
    const int k = blockIdx.x, tid = threadIdx.x;
    const SearchDesc sd = a.searches[k];
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const int p0 = sd.first_pair - a.sub_first_pair;
    for (int i = tid; i < lay.n_pairs; i += 256) a.audit_mark[p0 + i] = 0;
    if (tid == 0) { a.gkeys[a.first_search + k] = a.tkey; a.flags[a.first_search + k] = a.stamp; }
    __syncthreads();
    unsigned long long prev = 0ull;
    int n = 0;
    for (int j = 0; j < a.k + BEST_SEED_EXTRA; ++j) {
        unsigned long long best = NO_KEY;
        for (int i = tid; i < lay.n_pairs; i += 256) {
            // order-preserving key of a float that may be negative or -inf (pilot_kernel's)
            const unsigned b = __float_as_uint(a.slb[p0 + i]);
            const unsigned ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
            const unsigned long long key = ((unsigned long long)ord << 32) | (unsigned)i;
            if ((j == 0 || key > prev) && key < best) best = key;
        }
        best = wave_min_u64(best);
        __syncthreads();
        if ((tid & 63) == 0) red[tid >> 6] = best;
        __syncthreads();
        best = red[0];
        for (int w = 1; w < 4; ++w) best = red[w] < best ? red[w] : best;
        if (best == NO_KEY) break;                                          // (uniform) fewer pairs than that
        prev = best;
        const int pr = p0 + (int)(best & 0xffffffffull);
        if (tid == 0 && !best_excluded(a, pr, k)) {
            a.audit_mark[pr] = 2;
            a.list[atomicAdd(a.list_count, 1)] = pr;
            ++n;
        }
    }
    if (tid == 0 && n) atomicAdd(&a.counters->pairs_transformed, (unsigned long long)n);
}

// every pair not yet evaluated that its search's U does not exclude: listed, evaluated from now on, its search stamped
__global__ __launch_bounds__(256)
void best_survivor_kernel(BestArgs a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    bool add = false;
    int pr = 0;
    if (b < a.n_pairs) {
        pr = a.order[b];
        const int k = a.pairmap[pr];
        if (!(a.audit_mark[pr] & 2) && !best_excluded(a, pr, k)) {
            add = true;
            a.audit_mark[pr] = 2;
            a.flags[a.first_search + k] = a.stamp;
        }
    }
    best_append(a, add, pr);
}

// after the last round: a pair that would still be listed marks its search unsettled; an excluded pair that is its search's audit
// pair of this run (survivor_kernel's hash) is listed all the same
__global__ __launch_bounds__(256)
void best_final_kernel(BestArgs a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    bool add = false;
    int pr = 0;
    if (b < a.n_pairs) {
        pr = a.order[b];
        const int k = a.pairmap[pr];
        if (!(a.audit_mark[pr] & 2)) {
            if (!best_excluded(a, pr, k)) {
                a.need[a.first_search + k] = 1;
            } else if (a.audit_every > 0 && ((unsigned)(a.first_search + k) + a.audit_seq) % (unsigned)a.audit_every == 0u) {
                const SearchDesc sd = a.searches[k];
                const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
                const unsigned h = ((unsigned)(a.first_search + k) * 2654435761u + a.audit_seq * 40503u) >> 9;
                add = (int)(h % (unsigned)lay.n_pairs) == a.sub_first_pair + pr - sd.first_pair;
                if (add) a.audit_mark[pr] = 1 | 2 | 8;
            }
        }
    }
    best_append(a, add, pr);
}

// one thread per pair: an audited pair's bound against what the pair really scores (thr_check_kernel's test); the audit pair of
// the last stage must also hold nothing as good as its search's K-th pick.  A violated search is selected again over all its pairs.
__global__ __launch_bounds__(256)
void best_check_kernel(BestArgs a) {
    const int pr = blockIdx.x * 256 + threadIdx.x;
    if (pr >= a.n_pairs) return;
    const unsigned char am = a.audit_mark[pr];
    if (!(am & 1)) return;
    const int k = a.pairmap[pr];
    const uint32_t* __restrict__ row = a.rows + (size_t)pr * THR_SLOT_WORDS;
    float ub = __builtin_inff();
    for (int t = 0; t < TILES_PER_PAIR; ++t) ub = fminf(ub, __uint_as_float(row[THR_MIN + t]));
    // (TM_SQDIFF_NORMED scores are clamped at 1, cv2's rule, the bound is not)
    const float s = a.method == SUSHI_HIP_METHOD_CCOEFF_NORMED ? a.slb[pr] : fminf(a.slb[pr], 1.0f);
    const unsigned long long g = a.gkeys[a.first_search + k];
    const bool as_good = (am & 8) && g != NO_KEY && ub <= key_score(g);
    if (s > ub * 1.00001f + 1e-7f || as_good) {
        a.viol[a.first_search + k] = 1;
        a.flags[a.first_search + k] = a.stamp;
        atomicAdd(&a.counters->slb_violations, 1);
    }
    atomicAdd(&a.counters->excluded_audited, 1ull);
    const float ratio = s > 0.f ? s / fmaxf(ub, 1e-30f) : 0.f;
    atomicMax(&a.counters->max_slb_ratio_bits, __float_as_uint(ratio));
}

// every pair not yet evaluated of an unsettled or violated search
__global__ __launch_bounds__(256)
void best_extend_kernel(BestArgs a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    bool add = false;
    int pr = 0;
    if (b < a.n_pairs) {
        pr = a.order[b];
        const int k = a.first_search + a.pairmap[pr];
        if (!(a.audit_mark[pr] & 2) && (a.need[k] || a.viol[k])) {
            add = true;
            a.audit_mark[pr] |= 2;
            a.flags[k] = a.stamp;
        }
    }
    best_append(a, add, pr);
}
