// sushi_amd/csrc/sushi_fft_best.inc -- part of sushi_fft.hip (included there, inside its anonymous namespace; not a header of its own):
// the best-K run's own kernels (sushi_hip_batch_run_best, DESIGN.md 3.11).  The pair exclusion is the argmin run's (bound_excludes,
// is_audit_pair, append_pairs: sushi_fft_bound.inc; PairRunArgs, audit_pair: sushi_fft_threshold.inc), with the
// search's running threshold U FOUND by the run itself: the ranking score of the K-th pick that greedy suppression makes from the
// pairs evaluated so far (best_select_kernel, sushi_curve.hip, leaves it in gkeys).  A pair is listed for exact evaluation
// (best_tiles_kernel) as soon as its bound does not exclude it under the U of the moment, and a pair once evaluated stays so:
// audit_mark's MARK_LISTED.  Per sub-batch, a fixed launch sequence, every list length a count on the device:
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

struct BestArgs : PairRunArgs {       // (audit_mark: MARK_SECOND_LOOK by the second look, MARK_BEST_FINAL by best_final_kernel)
    int k;
    const int* order;                 // the L2-friendly schedule of all pairs (lists keep its order)
    unsigned long long* gkeys;        // [all searches]
    unsigned long long tkey;          // the threshold as a search key, NO_KEY: none
    int* list; int* list_count;
    int* flags;                       // [all searches] the stamp of the last round that evaluated a pair of the search
    int stamp;
    int* need;                        // [all searches] 1: unsettled after the last round
    unsigned audit_seq; int audit_every;
};

// one workgroup per search: no pair evaluated yet, U = the threshold's (or none); then the pairs of smallest bound are listed, one
// per round in (bound, pair) order -- "no bound" (-inf) first --, except those the threshold already excludes
__global__ __launch_bounds__(256)
void best_seed_kernel(BestArgs a) {
    __shared__ unsigned long long red[4];
    const int k = blockIdx.x, tid = threadIdx.x;
    const SearchDesc sd = a.searches[k];
    const FftLayout lay = fft_layout(sd.win_start, sd.n_pos, sd.tmpl_len);
    const int p0 = first_pair_in_sub(a.sub_first_pair, sd);
    for (int i = tid; i < lay.n_pairs; i += 256) a.audit_mark[p0 + i] = 0;
    if (tid == 0) { a.gkeys[a.first_search + k] = a.tkey; a.flags[a.first_search + k] = a.stamp; }
    __syncthreads();
    unsigned long long prev = 0ull;
    int n = 0;
    for (int j = 0; j < a.k + BEST_SEED_EXTRA; ++j) {
        unsigned long long best = NO_KEY;
        for (int i = tid; i < lay.n_pairs; i += 256) {
            // (pilot_kernel's key: a bound may be negative or -inf)
            const unsigned long long key = ((unsigned long long)ordered_bits(a.slb[p0 + i]) << 32) | (unsigned)i;
            if ((j == 0 || key > prev) && key < best) best = key;
        }
        best = block_min_u64(best, red);
        if (best == NO_KEY) break;                                          // (uniform) fewer pairs than that
        prev = best;
        const int pr = p0 + (int)(best & 0xffffffffull);
        if (tid == 0 && !bound_excludes(a.slb, pr, a.gkeys[a.first_search + k])) {
            a.audit_mark[pr] = MARK_LISTED;
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
        if (!(a.audit_mark[pr] & MARK_LISTED) && !bound_excludes(a.slb, pr, a.gkeys[a.first_search + k])) {
            add = true;
            a.audit_mark[pr] = MARK_LISTED;
            a.flags[a.first_search + k] = a.stamp;
        }
    }
    append_pairs(a.list, a.list_count, a.counters, add, pr);
}

// after the last round: a pair that would still be listed marks its search unsettled; an excluded pair that is its search's audit
// pair of this run (is_audit_pair: the pair survivor_kernel would audit) is listed all the same
__global__ __launch_bounds__(256)
void best_final_kernel(BestArgs a) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    bool add = false;
    int pr = 0;
    if (b < a.n_pairs) {
        pr = a.order[b];
        const int k = a.pairmap[pr];
        if (!(a.audit_mark[pr] & MARK_LISTED)) {
            if (!bound_excludes(a.slb, pr, a.gkeys[a.first_search + k])) {
                a.need[a.first_search + k] = 1;
            } else if (is_audit_pair(a, pr, k)) {
                add = true;
                a.audit_mark[pr] = MARK_AUDITED | MARK_LISTED | MARK_BEST_FINAL;
            }
        }
    }
    append_pairs(a.list, a.list_count, a.counters, add, pr);
}

// one thread per pair: an audited pair's bound against what the pair really scores (audit_pair); the audit pair of the last stage
// must also hold nothing as good as its search's K-th pick.  A violated search is selected again over all its pairs.
__global__ __launch_bounds__(256)
void best_check_kernel(BestArgs a) {
    const int pr = blockIdx.x * 256 + threadIdx.x;
    if (pr >= a.n_pairs) return;
    const unsigned char am = a.audit_mark[pr];
    if (!(am & MARK_AUDITED)) return;
    const int gk = a.first_search + a.pairmap[pr];
    const bool violated = audit_pair(a, pr, true, [&](const float ub) {
        const unsigned long long g = a.gkeys[gk];
        return (am & MARK_BEST_FINAL) && g != NO_KEY && ub <= key_score(g);
    });
    if (violated) a.flags[gk] = a.stamp;
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
        if (!(a.audit_mark[pr] & MARK_LISTED) && (a.need[k] || a.viol[k])) {
            add = true;
            a.audit_mark[pr] |= MARK_LISTED;
            a.flags[k] = a.stamp;
        }
    }
    append_pairs(a.list, a.list_count, a.counters, add, pr);
}
