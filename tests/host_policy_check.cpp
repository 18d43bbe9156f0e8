// What a run decides (sushi_amd/csrc/run_policy.hpp) on the CPU: every rule stated as checks, and scripted sequences of runs.
// usage: host_policy_check           checks every rule; exit 1 with a message on the first violation
//        host_policy_check --dump    drives a model of a batch handle -- the host steps of sushi_fft.hip around the rules, with the
//                                    device's answers (votes, counts) scripted -- through four scenarios: one JSON record per run and
//                                    line, with its inputs and every decision (tests/golden/policy_trace.json is this output):
//                                      "s" scenario, "seq" the run's sequence number,
//                                      "in"     [run kind, exclusion mode, method, votes: pairs looked at, with room, pairs listed per 1000, audited]
//                                      "form"   [counts absorbed, suspended, whole rows throughout, whole cut, lanes]
//                                      "subs"   per sub-batch [pairs, searches, excluded, voted, band, slots with a workgroup each or -1]
//                                      "learnt" [band, decided for method, votes x 2, suspended, suspended_at, last_transformed] after the run
//                                      "diag"   [band, suspended, votes x 2, pairs_transformed, second_look_audited] as the diagnostics report it
// Built by tests/test_policy_host.py with g++ -O2 -std=c++17, and once more with -O1 -g -fsanitize=address,undefined.
#include "../sushi_amd/csrc/sushi_geometry.hpp"
#include "../sushi_amd/csrc/run_policy.hpp"

#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

using namespace sushi;

namespace {

constexpr int AUTO = SUSHI_HIP_EXCLUDE_AUTO, ALWAYS = SUSHI_HIP_EXCLUDE_ALWAYS, NEVER = SUSHI_HIP_EXCLUDE_NEVER, BAND = SUSHI_HIP_EXCLUDE_BAND,
              WHOLE = SUSHI_HIP_EXCLUDE_WHOLE;
constexpr int SQDIFF = SUSHI_HIP_METHOD_SQDIFF_NORMED, CCOEFF = SUSHI_HIP_METHOD_CCOEFF_NORMED;
const int ALL_MODES[5] = {AUTO, ALWAYS, NEVER, BAND, WHOLE};

std::string g_rule;
#define REQUIRE(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s: %s -- ", g_rule.c_str(), #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

bool same(const Learnt& a, const Learnt& b) {
    return a.band == b.band && a.band_decided_method == b.band_decided_method && a.band_votes[0] == b.band_votes[0] &&
           a.band_votes[1] == b.band_votes[1] && a.suspended == b.suspended && a.suspended_at == b.suspended_at &&
           a.last_transformed == b.last_transformed;
}

// ---- the rules, one by one ----
void check_absorb_counts() {
    g_rule = "absorb_counts";
    const int64_t P = 4000;                                      // (0.75 P = 3000 exactly)
    Learnt l;
    absorb_counts(l, AUTO, 5, 3010, 10, P);                      // left == 0.75 P: not suspended
    REQUIRE(!l.suspended && l.suspended_at == 0 && l.last_transformed == 3010, "left == 0.75 P suspends");
    absorb_counts(l, AUTO, 6, 3011, 10, P);                      // one more: suspended, by the run that read it
    REQUIRE(l.suspended == 1 && l.suspended_at == 6 && l.last_transformed == 3011, "left == 0.75 P + 1 does not suspend");
    absorb_counts(l, AUTO, 70, 4000, 0, P);                      // a look-again run suspended again: suspended_at stays
    REQUIRE(l.suspended == 1 && l.suspended_at == 6, "suspended_at moved to %u", l.suspended_at);
    absorb_counts(l, AUTO, 134, 2999, 0, P);                     // it excluded well: the exclusion is back
    REQUIRE(!l.suspended && l.last_transformed == 2999, "a run that excluded well leaves the batch suspended");
    absorb_counts(l, AUTO, 200, 4000, 0, P);
    REQUIRE(l.suspended == 1 && l.suspended_at == 200, "a new suspension dates from %u", l.suspended_at);
    // every other mode records the count and never suspends
    for (const int mode : ALL_MODES) {
        if (mode == AUTO) continue;
        Learnt m;
        absorb_counts(m, mode, 9, 4000, 0, P);
        REQUIRE(!m.suspended && m.suspended_at == 0 && m.last_transformed == 4000, "mode %d", mode);
        m.suspended = 1; m.suspended_at = 3;                     // (left by AUTO before the mode changed: neither cleared nor used)
        absorb_counts(m, mode, 10, 1, 0, P);
        REQUIRE(m.suspended == 1 && m.suspended_at == 3 && m.last_transformed == 1 && !run_suspended(m, mode, 10), "mode %d", mode);
    }
}

void check_run_suspended() {
    g_rule = "run_suspended";
    Learnt l;
    for (unsigned r = 0; r < 200; ++r) REQUIRE(!run_suspended(l, AUTO, r), "run %u of a batch that is not suspended", r);
    const unsigned starts[] = {1u, 1000u, UINT_MAX - 200u, UINT_MAX - 62u, UINT_MAX};      // (the last three: run_seq wraps before the look-again)
    for (const unsigned s : starts) {
        l.suspended = 1; l.suspended_at = s;
        for (unsigned k = 0; k < 200; ++k) {
            const unsigned r = s + k;                            // unsigned: wraps as the handle's counter does
            const bool look = k == 63 || k == 127 || k == 191;
            REQUIRE(run_suspended(l, AUTO, r) == !look, "suspended at %u, run %u", s, r);
            for (const int mode : ALL_MODES) REQUIRE(mode == AUTO || !run_suspended(l, mode, r), "mode %d", mode);
        }
    }
}

void check_whole_rows() {
    g_rule = "whole_rows_throughout";
    for (const int mode : ALL_MODES)
        for (int band = -1; band <= 1; ++band)
            for (const int decided : {-1, SQDIFF, CCOEFF})
                for (const int method : {SQDIFF, CCOEFF})
                    for (int susp = 0; susp < (mode == AUTO ? 2 : 1); ++susp) {         // (only AUTO ever suspends a run)
                        Learnt l;
                        l.band = band; l.band_decided_method = decided;
                        const bool learnt_whole = (mode == AUTO || mode == ALWAYS) && band == 0 && decided == method;
                        const bool got = whole_rows_throughout(l, mode, method, susp != 0);
                        REQUIRE(got == (susp || mode == NEVER || mode == WHOLE || learnt_whole) && (mode != BAND || !got),
                                "mode %d band %d decided %d method %d suspended %d", mode, band, decided, method, susp);
                    }
    REQUIRE(takes_whole_cut(true, true) && !takes_whole_cut(true, false) && !takes_whole_cut(false, true) && !takes_whole_cut(false, false), "the cut");
    REQUIRE(run_lanes(true, 3) == 1 && run_lanes(false, 3) == 3 && run_lanes(false, 1) == 1, "the lanes");
}

void check_sub_excludes() {
    g_rule = "sub_excludes";
    for (const int n : {1, 24, 29, 3000})
        for (const int64_t d : {-1, 0, 1}) {
            const int64_t pairs = 3000 + 2 * (int64_t)n + d;
            REQUIRE(sub_excludes(AUTO, false, pairs, n) == (d > 0), "%d searches, %lld pairs", n, (long long)pairs);
            REQUIRE(!sub_excludes(AUTO, true, pairs, n), "a suspended run excludes");
            for (int susp = 0; susp < 2; ++susp) {
                REQUIRE(sub_excludes(ALWAYS, susp != 0, pairs, n) && sub_excludes(BAND, susp != 0, pairs, n) && sub_excludes(WHOLE, susp != 0, pairs, n), "a forced mode");
                REQUIRE(!sub_excludes(NEVER, susp != 0, pairs, n), "NEVER excludes");
            }
        }
    REQUIRE(sub_excludes(ALWAYS, false, 1, 1) && !sub_excludes(AUTO, false, 1, 1) && sub_excludes(AUTO, false, (int64_t)1 << 40, INT_MAX), "the extremes");
    for (const int mode : ALL_MODES) REQUIRE(listed_run_excludes(mode) == (mode != NEVER), "a listed run in mode %d", mode);
}

void check_form() {
    g_rule = "the form";
    // BAND / WHOLE: chosen by the caller, never a vote, Learnt untouched
    for (const int method : {SQDIFF, CCOEFF})
        for (int band = -1; band <= 1; ++band) {
            Learnt l;
            l.band = band; l.band_decided_method = band < 0 ? -1 : SQDIFF;
            const Learnt before = l;
            REQUIRE(!vote_due(l, BAND, method) && !vote_due(l, WHOLE, method), "a chosen form votes");
            REQUIRE(exclusion_form(l, BAND) == 1 && exclusion_form(l, WHOLE) == 0 && same(l, before), "a chosen form");
        }
    // the vote: v1 >= 0.75 v0, non-strict; no pairs looked at: whole rows
    const struct { int v0, v1, band; } votes[] = {{4000, 3000, 1}, {4000, 2999, 0}, {4000, 3001, 1}, {4000, 4000, 1}, {4000, 0, 0}, {0, 0, 0}, {1, 1, 1},
                                                  {1, 0, 0}, {3, 2, 0}, {4, 3, 1}, {INT_MAX, INT_MAX, 1}, {INT_MAX, INT_MAX / 4 * 3, 0}};
    for (const auto& v : votes) {
        Learnt l;
        decide_form(l, CCOEFF, v.v0, v.v1);
        REQUIRE(l.band == v.band && l.band_decided_method == CCOEFF && l.band_votes[0] == v.v0 && l.band_votes[1] == v.v1, "%d of %d votes", v.v1, v.v0);
    }
    // when a vote is due: none yet, or decided for another method -- and not again after it
    for (const int mode : {AUTO, ALWAYS}) {
        Learnt l;
        REQUIRE(vote_due(l, mode, SQDIFF) && vote_due(l, mode, CCOEFF), "a fresh batch");
        decide_form(l, SQDIFF, 100, 90);
        REQUIRE(!vote_due(l, mode, SQDIFF) && exclusion_form(l, mode) == 1, "decided for this method");
        REQUIRE(vote_due(l, mode, CCOEFF), "decided for SQDIFF, asked under CCOEFF");
        decide_form(l, CCOEFF, 100, 10);
        REQUIRE(!vote_due(l, mode, CCOEFF) && exclusion_form(l, mode) == 0 && vote_due(l, mode, SQDIFF), "after the new vote");
    }
}

void check_direct_slots() {
    g_rule = "direct_slots";
    // fewer pairs than the least grid: all of them, whatever is known
    for (const unsigned long long last : {0ull, 1ull, 100ull, 1000000ull}) REQUIRE(direct_slots(last, 4095, 4095) == 4095 && direct_slots(last, 1, 1) == 1, "p < 4096");
    // a first run (nothing known): half, at least 4096, at most all
    REQUIRE(direct_slots(0, 100000, 100000) == 50000 && direct_slots(0, 6000, 6000) == 4096 && direct_slots(0, 4096, 4096) == 4096, "a first run");
    // a last run that listed little: an eighth, at least 4096
    REQUIRE(direct_slots(1, 100000, 100000) == 12500 && direct_slots(12500, 100000, 100000) == 12500, "up to an eighth listed");
    REQUIRE(direct_slots(1, 20000, 20000) == 4096 && direct_slots(4096, 20000, 20000) == 4096, "up to the least grid listed");
    // ... more than that: every possible slot
    REQUIRE(direct_slots(12501, 100000, 100000) == 100000 && direct_slots(4097, 20000, 20000) == 20000, "more than an eighth listed");
    // two sub-batches of 60000 and 40000 pairs: each is held to ITS share of what the plan's last run listed
    const int64_t plan = 100000;
    REQUIRE(direct_slots(12500, 60000, plan) == 7500 && direct_slots(12500, 40000, plan) == 5000, "an eighth of the plan: 7500 and 5000 are the shares");
    REQUIRE(direct_slots(12501, 60000, plan) == 60000 && direct_slots(12501, 40000, plan) == 40000, "one pair more");
    // (the smaller one's grid is the least grid while its eighth is below it: its share may reach 4096, not 3750)
    REQUIRE(direct_slots(13653, 30000, plan) == 4096 && direct_slots(13654, 30000, plan) == 30000, "30000 of 100000: 4096 slots hold a share of 13653.3");
    REQUIRE(direct_slots(0, 60000, plan) == 30000 && direct_slots(0, 40000, plan) == 20000, "a first run, per sub-batch");
}

void check_records() {
    g_rule = "the records";
    Learnt l;
    decide_form(l, CCOEFF, 50, 49);
    absorb_counts(l, AUTO, 77, 1000, 1, 1000);
    REQUIRE(!same(l, Learnt()), "nothing was learnt");
    l.forget();
    REQUIRE(same(l, Learnt()) && l.band == -1 && l.band_decided_method == -1 && !l.suspended && l.last_transformed == 0, "forget() is not a fresh record");
    // what each run kind reports: a threshold or best-K run neither suspension nor votes nor the second look's audit
    RunCounters c;
    memset(&c, 0, sizeof(c));
    c.pairs_transformed = 700; c.second_look_audited = 9;
    decide_form(l, SQDIFF, 800, 700);
    for (const RunKind kind : {RUN_ARGMIN, RUN_THRESHOLD, RUN_BEST}) {
        LastRun last;
        REQUIRE(!last.ran, "a fresh handle has run");
        last.band = 0; last.whole_cut = true; last.suspended = true; last.direct_pairs = 5;      // (an earlier run's)
        begin_run(last, kind);
        REQUIRE(last.ran && last.kind == kind && last.band == -1 && !last.whole_cut && !last.suspended && last.direct_pairs == 0, "begin_run");
        last.band = 1; last.direct_pairs = 40; last.suspended = kind == RUN_ARGMIN;
        SushiHipBatchDiag d;
        memset(&d, 0, sizeof(d));
        report_last_run(last, l, c, &d);
        const bool argmin = kind == RUN_ARGMIN;
        REQUIRE(d.pairs_transformed == 740 && d.band == 1, "kind %d: %lld pairs, band %d", (int)kind, (long long)d.pairs_transformed, d.band);
        REQUIRE(d.suspended == (argmin ? 1 : 0) && d.band_votes[0] == (argmin ? 800 : 0) && d.band_votes[1] == (argmin ? 700 : 0) &&
                d.second_look_audited == (argmin ? 9 : 0), "kind %d", (int)kind);
    }
}

// ---- --dump: a model of a batch handle, driven through scripted runs ----
struct Sub { int64_t pairs; int n_sub; };
struct ModelPlan { std::vector<Sub> subs, subs_whole; int lanes; int64_t pairs; };

ModelPlan model_plan(std::vector<Sub> subs, int lanes, bool whole_cut) {
    ModelPlan p{subs, {}, lanes, 0};
    int n = 0;
    for (const Sub& s : subs) { p.pairs += s.pairs; n += s.n_sub; }
    if (whole_cut) p.subs_whole.push_back(Sub{p.pairs, n});
    return p;
}

// what the device answers in one run: the votes (read only when a vote is due) and, of the pairs that went through the exclusion,
// how many per thousand were listed and transformed, and how many excluded pairs were audited
struct Device { int votes_looked_at, votes_with_room, listed_per_mille, audited; };

struct Model {
    const char* scenario;
    ModelPlan plan;
    int exclusion, method = SQDIFF;
    unsigned run_seq = 0;
    Learnt learnt = {};
    LastRun last = {};
    bool stats_pending = false;
    unsigned long long host_stats[2] = {0, 0};

    // sushi_hip_batch_reset: the counts on their way are waited for and dropped, everything learnt is forgotten; run_seq goes on
    void reset(const ModelPlan& p) { stats_pending = false; plan = p; learnt.forget(); last = LastRun(); }

    void run(RunKind kind, const Device& dev) {
        begin_run(last, kind);
        const unsigned seq = run_seq++;
        const bool absorbed = kind == RUN_ARGMIN && stats_pending;      // (the model's event has always passed)
        bool suspended = false, whole_rows = false;
        const std::vector<Sub>* subs = &plan.subs;
        int lanes = plan.lanes;
        if (kind == RUN_ARGMIN) {                                // run_form
            if (absorbed) { stats_pending = false; absorb_counts(learnt, exclusion, seq, host_stats[0], host_stats[1], plan.pairs); }
            suspended = run_suspended(learnt, exclusion, seq);
            whole_rows = whole_rows_throughout(learnt, exclusion, method, suspended);
            last.suspended = suspended;
            last.whole_cut = takes_whole_cut(whole_rows, !plan.subs_whole.empty());
            if (last.whole_cut) subs = &plan.subs_whole;
            lanes = run_lanes(whole_rows, plan.lanes);
        }
        printf("{\"s\":\"%s\",\"seq\":%u,\"in\":[%d,%d,%d,%d,%d,%d,%d],\"form\":[%d,%d,%d,%d,%d],\"subs\":[", scenario, seq, (int)kind, exclusion, method,
               dev.votes_looked_at, dev.votes_with_room, dev.listed_per_mille, dev.audited, absorbed ? 1 : 0, suspended ? 1 : 0, whole_rows ? 1 : 0,
               last.whole_cut ? 1 : 0, lanes);
        RunCounters c;
        memset(&c, 0, sizeof(c));
        bool excluded_any = false;
        for (size_t si = 0; si < subs->size(); ++si) {
            const Sub& sb = (*subs)[si];
            const bool exclude = kind == RUN_ARGMIN ? sub_excludes(exclusion, suspended, sb.pairs, sb.n_sub) : listed_run_excludes(exclusion);
            bool voted = false;
            int band = 0;
            int64_t direct = -1;                                 // (-1: no listed transform)
            if (exclude) {
                excluded_any = true;
                voted = vote_due(learnt, exclusion, method);     // decide_band
                if (voted) decide_form(learnt, method, dev.votes_looked_at, dev.votes_with_room);
                band = last.band = exclusion_form(learnt, exclusion);
                if (kind == RUN_ARGMIN) direct = direct_slots(learnt.last_transformed, sb.pairs, plan.pairs);      // transform_listed
                c.pairs_transformed += (unsigned long long)(sb.pairs * dev.listed_per_mille / 1000);
                c.excluded_audited += (unsigned long long)dev.audited;
            } else {
                last.direct_pairs += sb.pairs;
            }
            printf("%s[%lld,%d,%d,%d,%d,%lld]", si ? "," : "", (long long)sb.pairs, sb.n_sub, exclude ? 1 : 0, voted ? 1 : 0, band, (long long)direct);
        }
        // sushi_hip_batch_run: what this run's exclusion left, for the runs after it
        if (kind == RUN_ARGMIN && excluded_any && !stats_pending) { host_stats[0] = c.pairs_transformed; host_stats[1] = c.excluded_audited; stats_pending = true; }
        SushiHipBatchDiag d;
        memset(&d, 0, sizeof(d));
        report_last_run(last, learnt, c, &d);
        printf("],\"learnt\":[%d,%d,%d,%d,%d,%u,%llu],\"diag\":[%d,%d,%d,%d,%lld,%lld]}\n",
               learnt.band, learnt.band_decided_method, learnt.band_votes[0], learnt.band_votes[1], learnt.suspended, learnt.suspended_at,
               learnt.last_transformed, d.band, d.suspended, d.band_votes[0], d.band_votes[1], (long long)d.pairs_transformed, (long long)d.second_look_audited);
    }
};

// tests/test_pair_exclusion.py test_auto_across_a_method_switch_a_suspension_and_the_look_again: 28 searches of about 121 pairs, none
// with a match anywhere (every pair is listed); two runs under SQDIFF, one under CCOEFF, then CCOEFF except every third run
void scenario_method_switch(const char* name, int exclusion) {
    Model m{name, model_plan({{3388, 28}}, 1, false), exclusion};
    for (int r = 0; r < 130; ++r) {
        m.method = r < 2 ? SQDIFF : r == 2 ? CCOEFF : r % 3 ? CCOEFF : SQDIFF;
        // (SQDIFF's vote takes the band-split form, CCOEFF's -- 2500 of 3388 -- the whole rows)
        m.run(RUN_ARGMIN, m.method == SQDIFF ? Device{3388, 3100, 998, 6} : Device{3388, 2500, 998, 6});
    }
}

// a batch on two lanes, its run_seq about to wrap: nothing can be excluded at first (a dub's silence), the look-again run excludes
// well and the exclusion is back -- on the lanes, then (CCOEFF's vote: whole rows) in the one-sub-batch cut without a suspension;
// later it is suspended anew, by a run whose number has wrapped
void scenario_recovers() {
    Model m{"recovers", model_plan({{5000, 40}, {3600, 24}}, 2, true), AUTO};
    m.run_seq = UINT_MAX - 66u;
    for (int r = 0; r < 74; ++r) {
        m.method = r >= 66 ? CCOEFF : SQDIFF;
        const bool poor = r < 3 || r >= 69;
        m.run(RUN_ARGMIN, Device{8600, m.method == SQDIFF ? 8000 : 1000, poor ? 990 : 80, 12});
    }
}

// a reset in the middle, and the other run kinds: runs of a plan below AUTO's limit, a new plan above it, a threshold and a best-K
// run between argmin runs, the mode changed on the way
void scenario_reset() {
    Model m{"reset", model_plan({{3050, 25}}, 1, false), AUTO};
    const Device dev{4000, 3000, 995, 3};
    for (int r = 0; r < 3; ++r) m.run(RUN_ARGMIN, dev);          // 3050 == 3000 + 2 * 25: no exclusion
    m.reset(model_plan({{3051, 25}}, 1, false));
    for (int r = 0; r < 4; ++r) m.run(RUN_ARGMIN, dev);          // one pair more: tried, then suspended
    m.run(RUN_THRESHOLD, dev);
    m.run(RUN_ARGMIN, dev);
    m.run(RUN_BEST, dev);
    m.reset(model_plan({{4000, 30}, {4000, 30}}, 2, true));      // forgotten: tried again, from a first run's grid
    for (int r = 0; r < 3; ++r) m.run(RUN_ARGMIN, Device{4000, 2999, 100, 3});
    for (const int mode : {NEVER, BAND, WHOLE, ALWAYS, AUTO}) {
        m.exclusion = mode;
        m.run(RUN_ARGMIN, dev);
        m.run(RUN_THRESHOLD, dev);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const bool dumping = argc == 2 && !strcmp(argv[1], "--dump");
    if (argc != 1 && !dumping) { fprintf(stderr, "usage: %s [--dump]\n", argv[0]); return 2; }
    if (dumping) {
        scenario_method_switch("auto", AUTO);
        scenario_method_switch("always", ALWAYS);
        scenario_recovers();
        scenario_reset();
        return 0;
    }
    check_absorb_counts();
    check_run_suspended();
    check_whole_rows();
    check_sub_excludes();
    check_form();
    check_direct_slots();
    check_records();
    return 0;
}
