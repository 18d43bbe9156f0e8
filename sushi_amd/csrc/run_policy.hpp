// sushi_amd/csrc/run_policy.hpp -- what a run of the FFT path DECIDES, host only: no HIP header, no environment, no globals.
// Every rule is a function of the exclusion mode, the method, a few counts and what earlier runs left behind; sushi_fft.hip makes
// the HIP calls around them (the event query, the vote's read-back, the uploads, the launches).  Built with plain g++ by
// tests/host_policy_check.cpp, which states the rules as checks on the CPU; sushi_fft.hip includes the same file.
//   Learnt                        what a batch has learnt about its searches
//   LastRun                       what its last run was (what the diagnostics entry points read)
//   absorb_counts, run_suspended  AUTO suspends an exclusion that excludes next to nothing, and looks again
//   whole_rows_throughout, takes_whole_cut, run_lanes     which cut of the plan a run takes, on how many lanes
//   sub_excludes, listed_run_excludes                     does a sub-batch go through the exclusion
//   vote_due, decide_form, exclusion_form                 band-split or whole rows
//   direct_slots                  slots of a listed transform that get a workgroup each
//   pilot_rows_route, pilot_rows_by_search                how the band-split form's pilots get their whole rows
//   rest_rows_route, rest_rows_by_item                    the unit of work of the survivors' pass behind them
//   slb_route, slb_by_wave                                how many lanes put a pair's lower bound together
//   second_look_route, second_look_plain                  which body the second look's transform kernel has
//   rest_pair_to_form, rest_item_starts, rest_item_take   how a search's surviving pairs are cut into that pass's work items
//   tspec_route, tspec_real                               which transform the pattern segments' spectra come from
//                                                         (the three the device calls as well: SUSHI_HHD)
//   begin_run, report_last_run    what a handle remembers of a run, what each run kind reports
#ifndef SUSHI_RUN_POLICY_HPP
#define SUSHI_RUN_POLICY_HPP

#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "sushi_geometry.hpp"

#ifndef SUSHI_HHD
#ifdef __HIPCC__
#define SUSHI_HHD __host__ __device__ inline
#else
#define SUSHI_HHD inline
#endif
#endif

namespace sushi {

enum RunKind { RUN_ARGMIN, RUN_THRESHOLD, RUN_BEST };

// What the batch has learnt about its searches (a new plan: about other searches now).
struct Learnt {
    int band = -1;                      // the exclusion's form in AUTO / ALWAYS: -1 not decided yet, 0 whole rows (bound_kernel), 1 band-split
    int band_decided_method = -1;       // ... which was decided for this method (the pattern spectra differ)
    int band_votes[2] = {0, 0};         // what the decision was taken from: pairs looked at, pairs whose bound leaves room
    // AUTO learns from its own runs: a batch whose exclusion excluded next to nothing (searches without a match anywhere) runs
    // without it from then on, looking again every 64th run.
    int suspended = 0;                  // 1: the exclusion is left out (AUTO)
    unsigned suspended_at = 0;          // run_seq of the run that showed it
    unsigned long long last_transformed = 0;    // pairs the last finished run transformed (0: not known): sizes the next run's one-workgroup-per-slot launch
    void forget() { *this = Learnt(); }
};

// What the last run was.
struct LastRun {
    RunKind kind = RUN_ARGMIN;          // (a best-K run's flags words hold, per search, the last round that evaluated a pair of it)
    int band = -1;                      // form of the exclusion it used (its last sub-batch that went through it; -1: none did)
    bool whole_cut = false;             // it took the plan's one-sub-batch cut (Plan::subs_whole)
    bool suspended = false;             // it was one of the runs AUTO leaves the exclusion out of
    int64_t direct_pairs = 0;           // pairs of its sub-batches that were transformed without the exclusion
    bool ran = false;
};

// (three quarters: a batch HALF of whose searches find nothing -- a dub -- still gains from the exclusion on the other half)
constexpr double SUSPEND_LEFT_SHARE = 0.75;
// (suspended: every 64th run looks again)
constexpr unsigned LOOK_AGAIN_MASK = 63u;
// The exclusion costs a pass over Y (~16 ns per pair) and half a dozen launches (~60 us); transforming a pair ~37 ns:
// it pays from ~3000 pairs on, plus two per search (the pairs transformed first are transformed either way).
constexpr int64_t EXCLUDE_FROM_PAIRS = 3000, EXCLUDE_PAIRS_PER_SEARCH = 2;
// (measured at BASELINE configs[2]: 97 % of the pairs vote for it at 12 dB of noise on the source -- 9.7 ms against 17.5 for
// the whole-row form --, 87 % at 6 dB -- 12.5 against 17.5 --, 14 % at 0 dB -- 28.7 against 18.7)
constexpr double BAND_VOTE_SHARE = 0.75;
// One workgroup per list slot up to what the list usually holds (an eighth of the pairs: empty slots there cost a
// workgroup's launch each, ~1 ns), and a fixed grid striding over whatever lies beyond: the striding form alone runs
// at half the rate per pair (the loop costs it registers), one workgroup per POSSIBLE slot cost 0.3 ms of empty launches.
constexpr int64_t DIRECT_SLOTS_MIN = 4096, DIRECT_USUAL_PART = 8;
// (nothing known yet -- a batch's first run, which is all a one-shot job has --: half of the pairs get a workgroup each;
// 0.15 ms of empty launches where there is a match everywhere, against half the rate on ten times as many pairs where
// there is not: a dub's first run 29.7 ms)
constexpr int64_t DIRECT_FIRST_RUN_PART = 2;

// The counts of a finished run (pairs transformed, excluded pairs audited), read by run `run_seq` of a plan of `plan_pairs`.
inline void absorb_counts(Learnt& l, int exclusion, unsigned run_seq, unsigned long long transformed, unsigned long long audited,
                          int64_t plan_pairs) {
    const unsigned long long left = transformed - audited;
    l.last_transformed = transformed;
    if (exclusion == SUSHI_HIP_EXCLUDE_AUTO) {
        if ((double)left > SUSPEND_LEFT_SHARE * (double)plan_pairs) { if (!l.suspended) l.suspended_at = run_seq; l.suspended = 1; }
        else l.suspended = 0;
    }
}

// Does AUTO leave the exclusion out of run `run_seq`.
inline bool run_suspended(const Learnt& l, int exclusion, unsigned run_seq) {
    return exclusion == SUSHI_HIP_EXCLUDE_AUTO && l.suspended && ((run_seq - l.suspended_at) & LOOK_AGAIN_MASK) != LOOK_AGAIN_MASK;
}

// The lanes: the batch's own streams start behind the fill, the caller's stream goes on behind them.  Side by side pays
// where the stages differ in what bounds them -- the band-split form; whole rows for every pair (the whole-row form, no
// exclusion at all) are HBM traffic from the first kernel to the last and only contend: those runs keep their sub-batches on
// the caller's stream, one after the other (measured at BASELINE configs[2]: unrelated audio 25.1 ms on one stream, 26.8 side by side).
inline bool whole_rows_throughout(const Learnt& l, int exclusion, int method, bool suspended) {
    return suspended || exclusion == SUSHI_HIP_EXCLUDE_NEVER || exclusion == SUSHI_HIP_EXCLUDE_WHOLE ||
           ((exclusion == SUSHI_HIP_EXCLUDE_AUTO || exclusion == SUSHI_HIP_EXCLUDE_ALWAYS) && l.band == 0 && l.band_decided_method == method);
}
inline bool takes_whole_cut(bool whole_rows, bool whole_cut_exists) { return whole_rows && whole_cut_exists; }
inline int run_lanes(bool whole_rows, int plan_lanes) { return whole_rows ? 1 : plan_lanes; }

// Does a sub-batch of `pairs` pairs and `n_sub` searches go through the exclusion (an argmin run).
inline bool sub_excludes(int exclusion, bool suspended, int64_t pairs, int n_sub) {
    return exclusion == SUSHI_HIP_EXCLUDE_ALWAYS || exclusion == SUSHI_HIP_EXCLUDE_BAND || exclusion == SUSHI_HIP_EXCLUDE_WHOLE ||
           (exclusion == SUSHI_HIP_EXCLUDE_AUTO && !suspended && pairs > EXCLUDE_FROM_PAIRS + EXCLUDE_PAIRS_PER_SEARCH * (int64_t)n_sub);
}

// ... and a sub-batch of a threshold or best-K run: every pair is listed or excluded on its bound alone, whatever the batch's size.
inline bool listed_run_excludes(int exclusion) { return exclusion != SUSHI_HIP_EXCLUDE_NEVER; }

// Which form of the exclusion: chosen by the caller (BAND / WHOLE), or decided once per batch and method by a
// vote of the pairs -- due while there is none, or none for this method.
inline bool form_chosen(int exclusion) { return exclusion == SUSHI_HIP_EXCLUDE_BAND || exclusion == SUSHI_HIP_EXCLUDE_WHOLE; }
inline bool vote_due(const Learnt& l, int exclusion, int method) {
    return !form_chosen(exclusion) && (l.band < 0 || l.band_decided_method != method);
}
inline void decide_form(Learnt& l, int method, int looked_at, int with_room) {
    l.band_votes[0] = looked_at; l.band_votes[1] = with_room;
    l.band = l.band_votes[0] > 0 && (double)l.band_votes[1] >= BAND_VOTE_SHARE * (double)l.band_votes[0] ? 1 : 0;
    l.band_decided_method = method;
}
inline int exclusion_form(const Learnt& l, int exclusion) {
    return !form_chosen(exclusion) ? l.band : exclusion == SUSHI_HIP_EXCLUDE_BAND ? 1 : 0;
}

// How many of a listed transform's `pairs` possible slots get a workgroup each (the comments at DIRECT_SLOTS_MIN).
// (A batch whose LAST run listed more than an eighth -- searches without a match, a dub's own speech -- gets a workgroup per
// possible slot instead: 0.3 ms of empty launches at most, against half the rate on everything behind the first eighth.
// `ifft` took 31.6 ms at BASELINE configs[2] on a dub with TM_CCOEFF_NORMED, 160 k pairs listed: bench.py --source dub.)
inline int64_t direct_slots(unsigned long long last_transformed, int64_t pairs, int64_t plan_pairs) {
    int64_t direct64 = std::min<int64_t>(pairs, std::max<int64_t>(DIRECT_SLOTS_MIN, pairs / DIRECT_USUAL_PART));
    if ((double)last_transformed * (double)pairs > (double)direct64 * (double)plan_pairs) direct64 = pairs;   // (this sub-batch's share of it)
    else if (last_transformed == 0) direct64 = std::min<int64_t>(pairs, std::max<int64_t>(DIRECT_SLOTS_MIN, pairs / DIRECT_FIRST_RUN_PART));
    return direct64;
}

// How the band-split form's pilots get their whole rows in an argmin run.  BY_SEARCH (the default): a pass over the searches, each
// pattern's spectra read once for the pilot and for the search's audit pair -- known before anything is scored: a hash of the
// search and the run --, and the survivors' pass later reads only the searches the bound left something of.  LIST: every pilot
// pair by pair and the survivors' pass over every search, as before that pass existed; kept for A/B measurements on one build.
// `setting` is SUSHI_HIP_PILOT_ROWS as the environment holds it (NULL or empty: the default); -1: neither route's name.
enum { PILOT_ROWS_BY_SEARCH = 0, PILOT_ROWS_LIST = 1 };
inline int pilot_rows_route(const char* setting) {
    if (!setting || !*setting || !strcmp(setting, "search")) return PILOT_ROWS_BY_SEARCH;
    return !strcmp(setting, "list") ? PILOT_ROWS_LIST : -1;
}
inline bool pilot_rows_by_search(int route) { return route != PILOT_ROWS_LIST; }

// The unit of work of the survivors' pass behind a BY_SEARCH first pass (mac_rows_kernel).  BY_ITEM (the default): a few listed
// pairs of one search -- dense_search_kernel cuts every search's pairs to form into runs of at most REST_ITEM_PAIRS and lists the
// runs, a workgroup takes (run, 256 entries).  BY_SEARCH: (search, 256 entries), every listed pair of the search one after the
// other, as before the items existed; kept for A/B measurements on one build.  `setting` is SUSHI_HIP_REST_ROWS as the
// environment holds it (NULL or empty: the default); -1: neither route's name.
enum { REST_ROWS_BY_ITEM = 0, REST_ROWS_BY_SEARCH = 1 };
inline int rest_rows_route(const char* setting) {
    if (!setting || !*setting || !strcmp(setting, "items")) return REST_ROWS_BY_ITEM;
    return !strcmp(setting, "search") ? REST_ROWS_BY_SEARCH : -1;
}
inline bool rest_rows_by_item(int route) { return route != REST_ROWS_BY_SEARCH; }

// How many lanes put a pair's lower bound together (slb_kernel, slb_list_kernel).  GROUP (the default): sixteen, four pairs a wave,
// where the four pairs' patterns have up to sixteen segments; a wave a pair otherwise.  WAVE: a wave a pair throughout
// (slb_wave_kernel, slb_list_wave_kernel), as before the groups; every stored value has the same bits either way.  Kept for A/B
// measurements on one build and for the tests to compare with.  `setting` is SUSHI_HIP_SLB as the environment holds it (NULL or
// empty: the default); -1: neither route's name.
enum { SLB_BY_GROUP = 0, SLB_BY_WAVE = 1 };
inline int slb_route(const char* setting) {
    if (!setting || !*setting || !strcmp(setting, "group")) return SLB_BY_GROUP;
    return !strcmp(setting, "wave") ? SLB_BY_WAVE : -1;
}
inline bool slb_by_wave(int route) { return route == SLB_BY_WAVE; }

// The body of the second look's transform kernel.  AHEAD (the default): bound_low_exact_kernel -- the band's registers by their
// index, the next slot requested ahead, one barrier for the maximum.  PLAIN: the body before that one
// (bound_low_exact_plain_kernel), whose acc[2 pr] the default's equals bit for bit; kept for A/B measurements on one build and for
// the tests to compare with.  `setting` is SUSHI_HIP_SECOND_LOOK as the environment holds it (NULL or empty: the default); -1:
// neither route's name.
enum { SECOND_LOOK_AHEAD = 0, SECOND_LOOK_PLAIN = 1 };
inline int second_look_route(const char* setting) {
    if (!setting || !*setting || !strcmp(setting, "ahead")) return SECOND_LOOK_AHEAD;
    return !strcmp(setting, "plain") ? SECOND_LOOK_PLAIN : -1;
}
inline bool second_look_plain(int route) { return route == SECOND_LOOK_PLAIN; }

// THE CUT of a search's pairs into the survivors' pass's work items.  An item is a run of the search's pairs that holds at most
// REST_ITEM_PAIRS pairs TO FORM -- listed, and not the audit pair the first pass formed already --, named by its first such
// pair; a search with nothing to form has no item.  Every item re-reads its pattern's spectra (a few 64 KB rows of the short
// patterns where the cutting happens, L2-hot behind the item in front), so the constant trades an even launch against those
// reads: 2, 4 and 8 were measured (tools/experiments/README.md).
// (-DSUSHI_REST_ITEM_PAIRS=<n>: a library with another value, for those measurements)
#ifndef SUSHI_REST_ITEM_PAIRS
#define SUSHI_REST_ITEM_PAIRS 4
#endif
constexpr int REST_ITEM_PAIRS = SUSHI_REST_ITEM_PAIRS;
static_assert(REST_ITEM_PAIRS >= 1, "an item holds a pair");
// is pair `i` of its search (`listed`: its mark's MARK_LISTED bit; `audit`: the search's audit pair, -1: none) one to form
SUSHI_HHD bool rest_pair_to_form(int listed, int i, int audit) { return listed != 0 && i != audit; }
// The builder's half.  `form`: which of 64 consecutive pairs of a search are to form (bit j: the j-th of them), `before`: how many
// pairs to form the search holds in front of them -> the bits that START an item: every `per_item`-th pair to form, from the first.
SUSHI_HHD unsigned long long rest_item_starts(unsigned long long form, int before, int per_item) {
    unsigned long long starts = 0;
    int rank = before;
    for (unsigned long long m = form; m; m &= m - 1, ++rank)
        if (rank % per_item == 0) starts |= m & (~m + 1);
    return starts;
}
// The consumer's half, walking on from an item's first pair 64 pairs at a time: of the pairs to form `form` among the next 64,
// the ones that are still the item's, which has room for `room` more -> the first `room` of them.
SUSHI_HHD unsigned long long rest_item_take(unsigned long long form, int room) {
    unsigned long long take = 0;
    for (unsigned long long m = form; m && room > 0; m &= m - 1, --room) take |= m & (~m + 1);
    return take;
}

// Which transform tspec_kernel's rows come from.  REAL (the default): a segment is real input -- packed into half as many complex
// points, one half-size transform, unfolded (fft_core.hpp; tspec_real_kernel).  COMPLEX: the full-size complex transform with zero
// imaginary parts, as before the real route existed; kept for A/B measurements on one build.  Both leave the low rows and norms in
// the same place and format (the whole rows: tspec_half_rows below); stored halves may differ in their last bit.  `setting` is SUSHI_HIP_TSPEC as the environment holds it (NULL
// or empty: the default); -1: neither route's name.
enum { TSPEC_REAL = 0, TSPEC_COMPLEX = 1 };
inline int tspec_route(const char* setting) {
    if (!setting || !*setting || !strcmp(setting, "real")) return TSPEC_REAL;
    return !strcmp(setting, "complex") ? TSPEC_COMPLEX : -1;
}
inline bool tspec_real(int route) { return route != TSPEC_COMPLEX; }
// The stored format of the whole pattern rows belongs to the route.  The real route's rows are conjugate-symmetric word for word,
// so it stores HALF rows (fft_core.hpp "HALF ROWS") and every reader derives the other half; the complex route's are symmetric
// only up to their last bit and stay whole rows, read as they always were.
inline bool tspec_half_rows(int route) { return tspec_real(route); }

// What a handle notes when a run of `kind` starts: run_form fills in the cut and the suspension of an argmin run, the sub-batches
// that go through the exclusion its form and those that do not their pairs.
inline void begin_run(LastRun& last, RunKind kind) {
    last = LastRun();
    last.kind = kind; last.ran = true;
}

// What the diagnostics say of the last run besides its device counters `c`.
// (a threshold or best-K run: the bound's figures only -- its exact stage is not the search's)
inline void report_last_run(const LastRun& last, const Learnt& l, const RunCounters& c, SushiHipBatchDiag* diag) {
    const bool argmin = last.kind == RUN_ARGMIN;
    diag->pairs_transformed = (int64_t)c.pairs_transformed + last.direct_pairs;
    diag->band = last.band;
    diag->suspended = argmin && last.suspended ? 1 : 0;
    diag->band_votes[0] = argmin ? l.band_votes[0] : 0; diag->band_votes[1] = argmin ? l.band_votes[1] : 0;
    diag->second_look_audited = argmin ? (int64_t)c.second_look_audited : 0;
}

}  // namespace sushi
#endif
