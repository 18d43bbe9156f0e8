"""The pair exclusion's small per-pair passes against the routes they replace, bit for bit, on the MI355X:
  slb_kernel / slb_list_kernel    four pairs a wave, a group of sixteen lanes each, for patterns of up to 16 segments (a wave a pair
                                  from 17 on) against SUSHI_HIP_SLB=wave, a wave a pair throughout;
  bound_low_exact_kernel          the band's registers by their index, the next slot ahead, one barrier for the maximum, against
                                  SUSHI_HIP_SECOND_LOOK=plain;
  survivor_kernel, survivor2_kernel   one reservation of list entries a workgroup: the lists against the marks and the count words.
Nothing here has a tolerance: every comparison is of bits, of sorted index lists or of counters.  The bounds of the two routes are
compared on the SAME inputs -- the bound pass launched again, by either route, on what one run left (SearchBatch.bounds_again) --
because two runs never have them: see _bounds_on_the_same_inputs.

The material is sushi_amd.synth audio at 12 kHz, sixteen block pairs long, the source = the stream advanced by 27,000 samples plus
white noise at 20 dB; every search has its match in its window.  Patterns of 1, 3, 15, 16, 17, 20 and 35 segments (the groups take
a pair up to 16, a wave from 17 on; the 35's norms need the wave's second flight of segments) in windows of 1, 3, 4, 5 and more
pairs that start off the pair grid, the one-segment pattern's ending with the stream; and one more search of 1, 2, 3 or 4 pairs,
so that the four jobs' pair counts are 0, 1, 2 and 3 modulo the four pairs of a wave (asserted).  One sub-batch per batch
(asserted), so that the views cover every pair.  The lists are read with SUSHI_HIP_REST_ROWS=search, under which the survivors'
pass leaves the first list alone."""
import functools

import numpy as np
import pytest

import fft_stage_ref as R

pytestmark = pytest.mark.gpu
PAIR = R.STEP * R.B
RATE, SHIFT = 12000, 27000
N_SAMPLES = 16 * PAIR
# (segments, pairs of the window, the window's first pair); the last one is the job's own: 1 .. 4 pairs
SEARCHES = [(35, 10, 0), (20, 12, 0), (20, 11, 1), (17, 12, 1), (20, 12, 0), (17, 11, 1), (16, 5, 3), (15, 4, 5), (1, 1, 15), (3, 3, 7)]
EXTRA = (5, 9)                             # (segments, first pair) of the job's own search
JOBS = (1, 2, 3, 4)                        # its pairs
OLD = {"SUSHI_HIP_SLB": "wave", "SUSHI_HIP_SECOND_LOOK": "plain"}
MARK_AUDITED, MARK_LISTED = 1, 2
CASES = [(m, t, f) for m in ("sqdiff_normed", "ccoeff_normed") for t in ("u8", "f32") for f in ("band", "whole")]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _typed(x, dtype):
    return (x * 255 + 0.5).astype(np.uint8) if dtype == "u8" else x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _material(dtype):
    from sushi_amd import synth
    dst_pcm = synth.make_dst_pcm(33, RATE, seed=91)[:N_SAMPLES]
    src_pcm = synth.make_src_pcm(dst_pcm, SHIFT, seed=92)
    # the full range, as WavStream normalises a stream
    dst = _typed(np.clip(dst_pcm.astype(np.float64) / 32768.0 + 0.5, 0, 1), dtype)
    src = _typed(np.clip(src_pcm.astype(np.float64) / 32768.0 + 0.5, 0, 1), dtype)
    dst.setflags(write=False); src.setflags(write=False)
    return dst, src


@functools.lru_cache(maxsize=None)
def _requests(extra_pairs):
    """-> (offs, lens, wst, npos, pairs per search, segments per search)"""
    from sushi_amd import _native
    offs, lens, wst, npos, pairs, segs = [], [], [], [], [], []
    for k, (s, p, w) in enumerate(SEARCHES + [(EXTRA[0], extra_pairs, EXTRA[1])]):
        m = s * R.B - 777 if s > 1 else R.B - 100
        ws = w * PAIR + 1000 + 37 * k                                  # off the pair grid
        n_pos = (p - 1) * PAIR + 5000
        if (s, p) == (1, 1):
            n_pos = N_SAMPLES - m - ws + 1                              # to the stream's end
            assert ws + n_pos + m - 1 == N_SAMPLES
        q = ws + (PAIR + 3000 if p >= 2 else 2500)                     # the match: in the window's second pair, or its only one
        assert ws <= q <= ws + n_pos - 1 and q - SHIFT >= 0 and q + m <= N_SAMPLES and ws + n_pos + m - 1 <= N_SAMPLES
        lay = _native.fft_layout(ws, n_pos, m)
        assert (lay[0], lay[1]) == (p, s), (k, lay, p, s)
        offs.append(q - SHIFT); lens.append(m); wst.append(ws); npos.append(n_pos); pairs.append(p); segs.append(s)
    return offs, lens, wst, npos, pairs, segs


def test_the_jobs_are_what_the_passes_need():
    residues = set()
    for extra in JOBS:
        _, _, wst, _, pairs, segs = _requests(extra)
        residues.add(sum(pairs) % 4)
        assert {1, 3, 15, 16, 17, 20, 35} <= set(segs) and {1, 3, 4, 5} <= set(pairs)
        assert all(w % PAIR for w in wst)
    assert residues == {0, 1, 2, 3}


@functools.lru_cache(maxsize=None)
def _streams(dtype):
    from sushi_amd.device import DeviceStream
    dst, src = _material(dtype)
    return DeviceStream(dst), DeviceStream(src)


def _batch(monkeypatch, dtype, method, exclusion, extra, env):
    """a batch created under `env` (the routes are read when a batch is created) and nothing else of the passes' switches"""
    from sushi_amd.device import SearchBatch
    for var in ("SUSHI_HIP_SLB", "SUSHI_HIP_SECOND_LOOK", "SUSHI_HIP_REST_ROWS", "SUSHI_HIP_PILOT_ROWS", "SUSHI_HIP_TEST_BOUND_FAULT",
                "SUSHI_HIP_AUDIT_EVERY", "SUSHI_HIP_LANES", "SUSHI_HIP_BOUND_MODEL"):
        monkeypatch.delenv(var, raising=False)
    for var, value in env.items():
        monkeypatch.setenv(var, value)
    D, S = _streams(dtype)
    offs, lens, wst, npos, pairs, _ = _requests(extra)
    b = SearchBatch(D, S, offs, lens, wst, npos, path="fft", method=method, exclusion=exclusion)
    assert b.sub_batches == 1 and b.fft_pairs == sum(pairs)
    return b


def _argmin(b):
    b.run()
    idx, score = b.results()
    slb, acc = b.pair_bounds()
    return {"idx": idx.copy(), "score": _bits(score).copy(), "slb": _bits(slb).copy(), "acc": _bits(acc).copy(), "diag": b.diagnostics(),
            "state": b.exclusion_state()}


def _bounds_on_the_same_inputs(b, stored, band, what):
    """Both routes of the bound pass on what ONE run left in the workspace (SearchBatch.bounds_again): the same accumulators, norms
    and tables, bit for bit.  Two RUNS do not have the same inputs to the last bit, whatever their routes -- a pattern segment's
    norm outside the band is a sum its transform's waves add to with float atomics, and so is the whole-row form's accumulator --,
    and two batches on the routes before this change differ in the last bit of a few bounds for it (the band-split form: one to
    four of 82) or of half of them (the whole-row form).  -> the bounds, as bits."""
    wave = _bits(b.bounds_again(True)[0]).copy()
    group = _bits(b.bounds_again(False)[0]).copy()
    assert np.array_equal(group, wave), (what, np.flatnonzero(group != wave)[:8])
    # ... and they are the run's own: what it stored was made from these inputs, by the route the batch was created with
    assert np.array_equal(group, stored), (what, np.flatnonzero(group != stored)[:8])
    if band:
        # the list kernels, over the list the second look left: the listed pairs' bounds again, the others untouched
        wave_l = _bits(b.bounds_again(True, 1)[0]).copy()
        group_l = _bits(b.bounds_again(False, 1)[0]).copy()
        assert np.array_equal(group_l, wave_l) and np.array_equal(group_l, stored), (what, np.flatnonzero(group_l != wave_l)[:8])
    return group


def _votes_on_the_same_inputs(b, what):
    """the prediction pass (band == 2) by both routes: the votes' totals and every pair's bound"""
    slb_w, votes_w = b.bounds_again(True, 2)
    slb_g, votes_g = b.bounds_again(False, 2)
    assert votes_g == votes_w and votes_g[0] == b.fft_pairs and 0 <= votes_g[1] <= votes_g[0], (what, votes_g, votes_w)
    assert np.array_equal(_bits(slb_g), _bits(slb_w)), (what, np.flatnonzero(_bits(slb_g) != _bits(slb_w))[:8])
    return votes_g


def _same_run(new, old, what, band):
    """What two runs CAN be held to across the routes: the answers always (they are exact whatever is excluded); in the band-split
    form, whose first look stores its accumulators one wave a pair, also the second look's accumulators bit for bit and every
    decision taken from the bounds -- marks, pair_lb, lists, counters.  (The whole-row form's accumulators are float atomic sums:
    there two runs of one route already list different pairs now and then.)"""
    assert np.array_equal(new["idx"], old["idx"]) and np.array_equal(new["score"], old["score"]), what
    if not band:
        return
    assert np.array_equal(new["acc"], old["acc"]), (what, np.flatnonzero((new["acc"] != old["acc"]).any(axis=1))[:8])
    sn, so = new["state"], old["state"]
    assert np.array_equal(sn["marks"], so["marks"]), (what, np.flatnonzero(sn["marks"] != so["marks"])[:8])
    assert np.array_equal(_bits(sn["pair_lb"]), _bits(so["pair_lb"])), what
    for key in ("pairs_transformed", "excluded_audited", "second_look_audited", "slb_violations", "band", "flagged", "all_positions"):
        assert new["diag"][key] == old["diag"][key], (what, key, new["diag"][key], old["diag"][key])
    assert (sn["n_slist"], sn["n_slist2"]) == (so["n_slist"], so["n_slist2"]), what
    for name, count in (("slist", "n_slist"), ("slist2", "n_slist2")):
        assert sorted(sn[name][:sn[count]].tolist()) == sorted(so[name][:so[count]].tolist()), (what, name)


def _lists_are_the_marks(run, band, pairs, what):
    """the list the transforms take (the second look's in the band-split form) holds exactly the pairs marked as listed, each once,
    as many as its count word says; the first list holds them all"""
    st = run["state"]
    n1, n2 = st["n_slist"], st["n_slist2"]
    assert 0 <= n1 <= pairs and 0 <= n2 <= pairs, (what, n1, n2)
    first = sorted(st["slist"][:n1].tolist())
    assert len(set(first)) == n1 and (not first or (first[0] >= 0 and first[-1] < pairs)), (what, first)
    listed = np.flatnonzero(st["marks"] & MARK_LISTED).tolist()
    if band:
        final = sorted(st["slist2"][:n2].tolist())
        assert final == listed and set(final) <= set(first), (what, final, listed, first)
    else:
        assert first == listed and n2 == 0, (what, first, listed, n2)
    return n1, len(listed)


@pytest.mark.parametrize("method,dtype,form", CASES)
def test_every_stored_value_of_the_three_passes_keeps_its_bits(monkeypatch, method, dtype, form):
    """Argmin runs under both bound models, of the four jobs: bounds, accumulators, marks, pair_lb, counters, lists and results
    of the default routes against the routes before them; the lists against the marks."""
    band = form == "band"
    looked_twice = 0
    for extra in JOBS:
        rest = {"SUSHI_HIP_REST_ROWS": "search"}
        new_b = _batch(monkeypatch, dtype, method, form, extra, rest)
        old_b = _batch(monkeypatch, dtype, method, form, extra, dict(OLD, **rest))
        pairs = new_b.fft_pairs
        for model in ("worst_case", "statistical"):
            new_b.set_bound_model(model); old_b.set_bound_model(model)
            new, old = _argmin(new_b), _argmin(old_b)
            what = (method, dtype, form, extra, model)
            assert new["diag"]["band"] == (1 if band else 0), (what, new["diag"])
            assert model != "worst_case" or new["diag"]["slb_violations"] == 0, (what, new["diag"])
            _same_run(new, old, what, band)
            if model == "worst_case":
                first = new                                            # (the batch's first run: what a fresh batch's is compared with)
            _bounds_on_the_same_inputs(old_b, old["slb"], band, what)
            _bounds_on_the_same_inputs(new_b, new["slb"], band, what)
            n1, n_final = _lists_are_the_marks(new, band, pairs, what)
            _lists_are_the_marks(old, band, pairs, what)
            # the second look ran (the first list held at most a fifth of the pairs) and changed an accumulator's bits somewhere
            if band and n1 <= pairs // 5 and n1 > 0:
                looked_twice += 1
            print("\nbound passes %s %s %s job %d %s: %d pairs, first list %d, listed %d, pairs_transformed %d, finite bounds %d"
                  % (method, dtype, form, extra, model, pairs, n1, n_final, new["diag"]["pairs_transformed"],
                     int(np.isfinite(new["slb"].view(np.float32)).sum())))
            assert np.isfinite(new["slb"].view(np.float32)).sum() * 2 > pairs, what          # (the comparison is of real bounds)
        # the default survivors' pass on top of the same lists: the same answers
        plain = _argmin(_batch(monkeypatch, dtype, method, form, extra, {}))
        assert np.array_equal(plain["idx"], first["idx"]) and np.array_equal(plain["score"], first["score"]), (method, dtype, form, extra)
        assert not band or plain["diag"]["pairs_transformed"] == first["diag"]["pairs_transformed"]
        _votes_on_the_same_inputs(new_b, (method, dtype, form, extra))
    if band:
        assert looked_twice > 0, "no job's first list was short enough for the second look"


@pytest.mark.parametrize("method,dtype,form", CASES)
def test_threshold_and_best_runs_are_the_same(monkeypatch, method, dtype, form):
    new_b = _batch(monkeypatch, dtype, method, form, JOBS[0], {})
    old_b = _batch(monkeypatch, dtype, method, form, JOBS[0], OLD)
    new_b.run(); old_b.run()
    score = new_b.results()[1].astype(np.float64)
    # a threshold every search's match passes, and under which the long patterns' bounds exclude
    t = 0.5 if method == "ccoeff_normed" else float(score.max()) * 1.5
    got = {}
    for route, b in (("new", new_b), ("old", old_b)):
        hits, counts = b.run_threshold(t, 64)
        got[route, "thr"] = (hits.cpu().numpy().copy(), counts.cpu().numpy().copy(), b.diagnostics())
        hits, counts = b.run_best(2, 2000, None)
        got[route, "best2"] = (hits.cpu().numpy().copy(), counts.cpu().numpy().copy(), b.diagnostics())
    for kind in ("thr", "best2"):
        (h, c, d), (ho, co, do) = got["new", kind], got["old", kind]
        assert np.array_equal(c, co) and c.min() >= 1, (kind, c, co)
        for k in range(c.shape[0]):
            n = min(int(c[k]), h.shape[1])
            assert np.array_equal(h[k, :n], ho[k, :n]), (kind, k)
        assert d["slb_violations"] == do["slb_violations"] == 0, (kind, d, do)
        assert form != "band" or d["pairs_transformed"] == do["pairs_transformed"], (kind, d, do)


@pytest.mark.parametrize("method,dtype", [(m, t) for m in ("sqdiff_normed", "ccoeff_normed") for t in ("u8", "f32")])
def test_the_prediction_pass_counts_the_same_votes(monkeypatch, method, dtype):
    """exclusion='always': the batch's first run decides the exclusion's form from slb_kernel's prediction pass (band == 2)"""
    for extra in JOBS:
        new_b = _batch(monkeypatch, dtype, method, "always", extra, {})
        old_b = _batch(monkeypatch, dtype, method, "always", extra, OLD)
        new, old = _argmin(new_b), _argmin(old_b)
        votes, votes_old = new["diag"]["band_votes"], old["diag"]["band_votes"]
        assert votes == votes_old and votes[0] == new_b.fft_pairs and 0 <= votes[1] <= votes[0], (extra, votes, votes_old)
        assert new["diag"]["band"] == old["diag"]["band"]
        assert np.array_equal(new["idx"], old["idx"]) and np.array_equal(new["score"], old["score"])
        for b in (new_b, old_b):
            assert _votes_on_the_same_inputs(b, (method, dtype, extra)) == votes


def _audit_pair(g, seq, n_pairs):
    """the audit's hash (tests/test_bound_fault_gpu.py states the contract)"""
    return (((g * 2654435761 + seq * 40503) & 0xffffffff) >> 9) % n_pairs


@pytest.mark.parametrize("method,dtype,form", CASES)
def test_a_faulted_batch_still_recovers(monkeypatch, method, dtype, form):
    """SUSHI_HIP_TEST_BOUND_FAULT=3:0, every search audited every run: every pair of searches 0, 3, 6 and 9 carries a bound of +inf,
    the audit catches each of those searches in the run whose hashed pair is not the one transformed first (the first pair: all
    tie), and the run answers what the batch without the fault answers."""
    pairs = _requests(JOBS[0])[4]
    faulted = [g for g in range(len(pairs)) if g % 3 == 0]
    assert all(pairs[g] >= 2 for g in faulted)
    seq = next(s for s in range(64) if all(_audit_pair(g, s, pairs[g]) != 0 for g in faulted))
    control = _batch(monkeypatch, dtype, method, form, JOBS[0], {"SUSHI_HIP_AUDIT_EVERY": "1"})
    b = _batch(monkeypatch, dtype, method, form, JOBS[0], {"SUSHI_HIP_AUDIT_EVERY": "1", "SUSHI_HIP_TEST_BOUND_FAULT": "3:0"})
    for _ in range(seq):                                               # (the runs before: the batch's run counter feeds the hash)
        control.run(); b.run()
        control.diagnostics(); b.diagnostics()
    control.run(); b.run()
    want, got = control.results(), b.results()
    dc, d = control.diagnostics(per_search=True), b.diagnostics(per_search=True)
    assert dc["slb_violations"] == 0 and dc["all_positions"] == 0, dc
    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1])), (got[0], want[0])
    assert d["slb_violations"] >= len(faulted) and d["all_positions"] == len(faulted), d
    assert np.flatnonzero(d["flagged_per_search"] == 2).tolist() == faulted, d["flagged_per_search"]
