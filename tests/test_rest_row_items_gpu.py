"""The survivors' pass of the band-split form by work items (mac_rows_kernel, ROWS_ITEMS: dense_search_kernel cuts every search's
pairs to form into runs of at most C = REST_ITEM_PAIRS and lists them; a workgroup takes (item, 256 entries)) against the pass
it replaces (SUSHI_HIP_REST_ROWS=search: a workgroup per (search, 256 entries)) and against float64, on the MI355X.

The helpers are tests/test_pilot_audit_rows_gpu.py's and tests/test_fft_stages_gpu.py's: the sentinel procedure on WS_Y (which
rows a run wrote, none of them half), fft_stage_ref.product_mismatch (every written row against float64 from the stored factors)
and the audit's hash.  Every batch is one sub-batch (asserted there), exclusion="band", both methods, u8 and f32.

The material is sushi_amd.synth audio at 12 kHz, the source = the stream advanced by 27,000 samples plus noise, on the 8-bit
grid for both sample types (float32: level / 256), so that every float64 sum over it is exact and EXACT DUPLICATES of a matched
excerpt, planted later in its window, score exactly what the match scores: the first occurrence wins, each duplicate's pair ties
the search's threshold, and no sound bound can exclude it -- that is how a search gets a chosen number of pairs to form.  Every
excerpt starts well inside its pair (_inside).  The patterns of up to four segments, whose pairs the bound does not exclude in
ordinary material, get material of their own (_levels_a: the envelope taken out, quiet around them for TM_SQDIFF_NORMED).

  job A   180 s; windows of 40 pairs, the last one ending with the stream; patterns of 30, 19, 18, 7, 6, 4 and 1 segments with
          0, 1, C, C + 1, 2 C + 1, C and 1 duplicates: both instances of mac_rows_kernel and both edges of each.
  job B   one pattern of one segment in a window of 300 pairs (7.4 M samples), 65 duplicates, among them pairs 63, 64, 255, 256,
          the window's last pair and the audit pairs of the runs taken: the builder's and the consumer's 64-pair steps.
  job C   job A and searches for noise, which the bound excludes nothing of: two of them hold more than an eighth of the pairs and
          take the dense form next to job A's items; a lone one does not, dense_repack_kernel clears its flag, and all its pairs
          become items.

The oracle's index is the first extremum of its score row; where the row holds several within 1e-6 -- the duplicates: the
oracle's FFT route is not exact -- each of them is evaluated again on its own by the direct route and the first best one taken."""
import functools
import os
import re

import numpy as np
import pytest

import fft_stage_ref as R
import test_fft_stages_gpu as S
import test_pilot_audit_rows_gpu as P

pytestmark = pytest.mark.gpu
PAIR = S.PAIR
RATE, SHIFT = 12000, 27000
WINDOW = 40                                # pairs of a window of jobs A and C
MATCH_PAIR = 2                             # the pair of its window that holds a search's match (or the next one that no run taken audits)
with open(os.path.join(S.ROOT, "sushi_amd", "csrc", "run_policy.hpp")) as _f:
    C = int(re.search(r"#define SUSHI_REST_ITEM_PAIRS (\d+)", _f.read()).group(1))
A_SEGS = [30, 19, 18, 7, 6, 4, 1]          # the last search's window ends with the stream
A_DUPS = [0, 1, C, C + 1, 2 * C + 1, C, 1]
RUNS = {1: (1,), 2: (1, 2)}                # audit rate -> the sentinel runs taken (rate 2: both parities of the run number)


def _levels(pcm):
    """8-bit levels over the full range, as WavStream normalises a stream: clipped at three times the median magnitude, then scaled
    (a quieter stream on the same level leaves TM_SQDIFF_NORMED too little spread for the bound to exclude a short pattern's pairs)"""
    x = pcm.astype(np.float64)
    lim = 3.0 * float(np.median(np.abs(x)))
    return S._as((np.clip(x, -lim, lim) + lim) / (2.0 * lim), "u8", 1.0)


def _flat_levels(pcm):
    """... of the same material with synth.make_dst_pcm's slow envelope taken out again: the envelope is nearly silent every 1.25 s,
    twice in every pair, and a pair's bound stands on the QUIETEST window it holds -- next to silence no pair of a short pattern
    is ever excluded"""
    t = np.arange(pcm.shape[0], dtype=np.float64) / RATE
    return _levels(pcm.astype(np.float64) / (np.abs(np.sin(2 * np.pi * 0.2 * t)) + 0.1))


def _typed(levels, dtype):
    a = levels.copy() if dtype == "u8" else levels.astype(np.float32) / np.float32(256.0)
    a.setflags(write=False)
    return a


def _free(reserved, a, b):
    return all(b <= x or a >= y for x, y in reserved)


def _quiet(levels):
    """the same material at a twenty-fifth of its swing about the middle level"""
    return np.round(128.0 + (levels.astype(np.float64) - 128.0) * 0.04).astype(np.uint8)


def _inside(q):
    """an excerpt starts well inside its pair: a match a few samples behind a pair's last position still shows in that pair's
    transform (the outputs it discards), and its bound cannot exclude it"""
    return 5000 <= q % PAIR <= PAIR - 5000


def _plant(dst, excerpt, reserved, first, last_pos, taken, want):
    """Copies of `excerpt` into dst at the earliest free places from `first` on, each in another pair of the window that `taken`
    does not hold yet (its own pairs are added), none beyond position last_pos -> the pairs (absolute)."""
    pairs, q, m = [], first, excerpt.shape[0]
    while len(pairs) < want and q <= last_pos and q + m <= dst.shape[0]:
        if q // PAIR not in taken and _inside(q) and _free(reserved, q, q + m):
            dst[q:q + m] = excerpt
            reserved.append((q, q + m)); taken.add(q // PAIR); pairs.append(q // PAIR)
            q += m
        else:
            q += PAIR // 16
    assert len(pairs) == want, (m, want, pairs)
    return pairs


SHORT = 4                                  # patterns of up to this many segments: see _levels_a


@functools.lru_cache(maxsize=None)
def _levels_a(quiet):
    """-> (dst levels with the duplicates planted, src levels, offs, lens, wst, npos, per search the pairs of its window that hold
    a duplicate, per search the pair that holds its match).  The patterns of more than SHORT segments are cut from the noisy
    source and live in the first 48 pairs.  Among material as loud as itself no bound excludes the pairs of a SHORT pattern (the
    worst-case error terms and the coarse prefix table's granularity are a large part of so few samples' energy), so those two are
    passages of the stream's last 40 pairs, where the envelope is taken out (_flat_levels), and their source excerpts hold the same
    samples: the match scores exactly zero.  `quiet` (TM_SQDIFF_NORMED): the stream around them at a twenty-fifth of the swing
    (_quiet), so that the quiet pairs are excluded on the pattern's energy alone -- between equally loud rows the DC level the
    method keeps leaves the bound no room.  Not `quiet` (TM_CCOEFF_NORMED, which centres both sides): evenly loud material; quiet
    windows would leave the bound's error terms, which stand on the rows' uncentred norms, larger than the windows' own energy."""
    from sushi_amd import synth
    dst_pcm = synth.make_dst_pcm(180, RATE, seed=61)
    original, src = _levels(dst_pcm).copy(), _levels(synth.make_src_pcm(dst_pcm, SHIFT, seed=62)).copy()
    n = original.shape[0]
    original[48 * PAIR:] = _flat_levels(dst_pcm)[48 * PAIR:]          # where the short patterns' windows lie: evenly loud ...
    dst = original.copy()
    if quiet:
        dst[48 * PAIR:] = _quiet(original[48 * PAIR:])                  # ... and, but for their excerpts, quiet
    offs, lens, wst, npos, wpair, match, mpair, reserved = [], [], [], [], [], [], [], []
    for k, s in enumerate(A_SEGS):
        m = s * R.B - 777 if s > 1 else R.B            # (one whole segment: the coarse prefix table misses up to 512 samples of a window)
        if s > SHORT:
            w = 2 * k
            ws, p = w * PAIR + 1000, (WINDOW - 1) * PAIR + 5000
        else:
            w = (n - m) // PAIR - (WINDOW - 1)
            ws = w * PAIR + 1000
            p = n - m - ws + 1 if k == len(A_SEGS) - 1 else (WINDOW - 1) * PAIR + 5000      # the last window ends where the stream ends
        # the match: the first free place from the window's pair MATCH_PAIR on (the short patterns': apart from each other) that lies
        # in a pair no run taken audits
        audits = {P.audit_pair(k, seq, WINDOW) for seq in (1, 2)}
        pos = (w + MATCH_PAIR + (0 if s > SHORT else 6 * (k - 4))) * PAIR + 5000
        while pos // PAIR - w in audits or not _inside(pos) or not _free(reserved, pos, pos + m):
            pos += PAIR // 16
        reserved.append((pos, pos + m))
        if s <= SHORT:
            dst[pos:pos + m] = original[pos:pos + m]
            src[pos - SHIFT:pos - SHIFT + m] = dst[pos:pos + m]
        offs.append(pos - SHIFT); lens.append(m); wst.append(ws); npos.append(p); wpair.append(w); match.append(pos); mpair.append(pos // PAIR - w)
        assert pos - SHIFT >= 0 and pos - SHIFT + m <= n and ws + p + m - 1 <= n and w >= 0 and ws <= pos <= ws + p - 1
        assert (w >= 48) == (s <= SHORT)
    assert wst[-1] + npos[-1] + lens[-1] - 1 == n
    planted = []
    for k, d in enumerate(A_DUPS):
        m, w = lens[k], wpair[k]
        last_pos = wst[k] + npos[k] - 1
        taken = {w + P.audit_pair(k, seq, WINDOW) for seq in (1, 2)} | {w + mpair[k]}
        pairs = []
        if d and k == len(A_SEGS) - 1:                           # the stream's very last position: the window's last pair
            assert (last_pos // PAIR) - w == WINDOW - 1 and last_pos // PAIR not in taken
            dst[last_pos:last_pos + m] = dst[match[k]:match[k] + m]
            reserved.append((last_pos, last_pos + m)); taken.add(last_pos // PAIR); pairs.append(last_pos // PAIR)
        pairs += _plant(dst, dst[match[k]:match[k] + m].copy(), reserved, match[k] + m, last_pos, taken, d - len(pairs))
        planted.append(sorted(q - w for q in pairs))
        assert all(0 <= i < WINDOW for i in planted[-1])
    dst.setflags(write=False)
    return dst, src, offs, lens, wst, npos, planted, mpair


B_PAIRS = 300


@functools.lru_cache(maxsize=None)
def _levels_b(quiet):
    """one short pattern in a long window: a loud passage of a quiet stream (_levels_a), then its duplicates"""
    from sushi_amd import synth
    m = R.B
    n = PAIR + B_PAIRS * PAIR + m - 1
    dst_pcm = synth.make_dst_pcm(-(-n // RATE), RATE, seed=71)
    src = _levels(synth.make_src_pcm(dst_pcm, SHIFT, seed=72))[:n].copy()
    original = _flat_levels(dst_pcm)[:n]
    dst = _quiet(original) if quiet else original.copy()
    ws, p = PAIR, B_PAIRS * PAIR
    pos = ws + PAIR // 2
    pairs = {63, 64, 255, 256, B_PAIRS - 1} | {P.audit_pair(0, seq, B_PAIRS) for seq in (1, 2)} | set(range(5, B_PAIRS, 5))
    pairs -= {0}
    pairs = sorted(pairs)
    assert 60 <= len(pairs) <= 75 and (len(pairs) + 1) * 5 < B_PAIRS * 2
    dst[pos:pos + m] = original[pos:pos + m]
    src[pos - SHIFT:pos - SHIFT + m] = dst[pos:pos + m]
    excerpt = dst[pos:pos + m].copy()
    for i in pairs:
        q = ws + i * PAIR + PAIR // 2 + (i * 131) % 1000
        assert q + m <= n and q <= ws + p - 1
        dst[q:q + m] = excerpt
    return dst, src, [pos - SHIFT], [m], [ws], [p], [pairs], [0]


NOISE_LEN = 20000


@functools.lru_cache(maxsize=None)
def _levels_c(lone, quiet):
    dst, src, offs, lens, wst, npos, planted, mpair = _levels_a(quiet)
    rng = np.random.default_rng(81)
    windows = [(3, 30)] if lone else [(3, WINDOW), (7, WINDOW)]         # (among the long patterns: ordinary material)
    offs, lens, wst, npos, planted = list(offs), list(lens), list(wst), list(npos), list(planted)
    for w, pairs in windows:
        offs.append(src.shape[0]); lens.append(NOISE_LEN); wst.append(w * PAIR + 1000); npos.append((pairs - 1) * PAIR + 5000)
        planted.append(None)                                      # (a search for noise)
        src = np.concatenate([src, rng.integers(0, 256, NOISE_LEN).astype(np.uint8)])
    return dst, src, offs, lens, wst, npos, planted, mpair


LEVELS = {"A": _levels_a, "B": _levels_b, "C": functools.partial(_levels_c, False), "C-lone": functools.partial(_levels_c, True)}


def _made(name, method):
    """a job's levels for a method (the material around the short patterns differs: _levels_a)"""
    return LEVELS[name](method == "sqdiff_normed")


@functools.lru_cache(maxsize=None)
def _job(name, dtype, method):
    dst, src, offs, lens, wst, npos = _made(name, method)[:6]
    return _typed(dst, dtype), _typed(src, dtype), offs, lens, wst, npos


@functools.lru_cache(maxsize=None)
def _streams(name, dtype, method):
    from sushi_amd.device import DeviceStream
    job = _job(name, dtype, method)
    D, Sx = DeviceStream(job[0]), DeviceStream(job[1])
    z_c = R.complex_of_words(R.words(D.spectra(), R.N))
    z_c.setflags(write=False)
    return D, Sx, z_c


@functools.lru_cache(maxsize=None)
def _oracle_index(name, dtype, method):
    from oracle import oracle as O
    O.build()
    dst, src, offs, lens, wst, npos = _job(name, dtype, method)
    cc = method == "ccoeff_normed"
    out = []
    for o, m, w, p in zip(offs, lens, wst, npos):
        t = src[o:o + m]
        row = np.asarray(O.match_template(dst[w:w + p + m - 1], t, corr_f32=False, method=method)[0], np.float64)
        best = row.max() if cc else row.min()
        cand = np.flatnonzero(np.abs(row - best) <= 1e-6)
        if cand.size > 1:
            exact = np.array([float(O.match_template_direct(dst[w + q:w + q + m], t, False, method)[0][0]) for q in cand])
            cand = cand[np.flatnonzero(exact == (exact.max() if cc else exact.min()))]
        out.append(int(cand[0]))
    return out


def _batch(name, dtype, method, exclusion):
    from sushi_amd.device import SearchBatch
    D, Sx, _ = _streams(name, dtype, method)
    _, _, offs, lens, wst, npos = _job(name, dtype, method)
    return SearchBatch(D, Sx, offs, lens, wst, npos, path="fft", method=method, exclusion=exclusion)


def _geometry(lib, job):
    _, _, offs, lens, wst, npos = job
    out, pr0 = [], 0
    for w, p, m in zip(wst, npos, lens):
        _, n_pairs, n_seg = S._pairs_of(lib, w, p, m)
        out.append((pr0, n_pairs, n_seg))
        pr0 += n_pairs
    return out


@pytest.fixture(scope="module")
def lib():
    from sushi_amd import _native
    L = _native.lib()
    assert (L.sushi_hip_fft_size(), L.sushi_hip_fft_block()) == (R.N, R.B)
    return L


def _behind(geo, written, seq, every):
    """per search: the rows written behind its first pass -- every written row but the audit pair's (an audited search's) and the
    pilot's (no job plants on an audit pair of the runs taken but job B, whose one search is not asked for a count)"""
    out = []
    for g, (p0, n_pairs, _) in enumerate(geo):
        rows = set(np.flatnonzero(written[p0:p0 + n_pairs]).tolist())
        if P.audited(g, seq, every):
            rows.discard(P.audit_pair(g, seq, n_pairs))
        out.append(len(rows) - 1)
    return out


def _both_routes(lib, monkeypatch, name, method, dtype, every):
    """Both routes' sentinel runs of one job, with every assertion the jobs share; -> (geometry, the `search` route's runs)."""
    from sushi_amd import _native
    job = _job(name, dtype, method)
    geo = _geometry(lib, job)
    z_c = _streams(name, dtype, method)[2]
    scales = S._host_mac_scales(job, method)
    for var in ("SUSHI_HIP_TEST_BOUND_FAULT", "SUSHI_HIP_PILOT_ROWS", "SUSHI_HIP_REST_ROWS"):
        monkeypatch.delenv(var, raising=False)
    never = _batch(name, dtype, method, "never")
    never.run()
    want = P._result(never)
    assert want[0] == _oracle_index(name, dtype, method), (want[0], _oracle_index(name, dtype, method))
    monkeypatch.setenv("SUSHI_HIP_AUDIT_EVERY", str(every))
    got = {}
    for route in ("items", "search"):
        if route == "search":
            monkeypatch.setenv("SUSHI_HIP_REST_ROWS", "search")
        b = _batch(name, dtype, method, "band")
        got[route] = P._sentinel_runs(b, len(RUNS[every]))            # (one sub-batch, band-split form, no half-written row)
        assert b.fft_pairs == sum(n for _, n, _ in geo)
        if route == "items":
            u_c = R.complex_of_words(R.words(b.workspace_view(_native.WS_TSPEC), R.N))
            for seq, res, d, written, yw in got[route]:
                assert P._check_rows(geo, lib, job, yw, z_c, u_c, written, scales, "Y rows, job %s run %d" % (name, seq)) == written.sum()
    for (seq, res, d, written, yw), (seq_s, res_s, d_s, written_s, yw_s) in zip(got["items"], got["search"]):
        assert seq == seq_s and seq in RUNS[every]
        extra, missing = np.flatnonzero(written & ~written_s), np.flatnonzero(written_s & ~written)
        print("\nrest row items %s %s %s every %d run %d: rows written %d (search route %d; only here %s, only there %s), behind the first pass "
              "per search %s, pairs_transformed %d / %d, excluded_audited %d / %d, flagged %d, slb_violations %d"
              % (name, method, dtype, every, seq, int(written.sum()), int(written_s.sum()), extra.tolist(), missing.tolist(),
                 _behind(geo, written_s, seq, every), d["pairs_transformed"], d_s["pairs_transformed"], d["excluded_audited"],
                 d_s["excluded_audited"], d["flagged"], d["slb_violations"]))
        assert res == want and res_s == want, (seq, res[0], res_s[0], want[0])
        assert d["slb_violations"] == 0 and d["flagged"] == 0 and d_s["slb_violations"] == 0 and d_s["flagged"] == 0, (d, d_s)
        assert extra.size == 0 and missing.size == 0, (extra.tolist(), missing.tolist())       # the same rows under both routes ...
        assert (yw[written] == yw_s[written]).all(), (seq, np.flatnonzero((yw[written] != yw_s[written]).any(axis=1)))   # ... the same words
        assert d["pairs_transformed"] == d_s["pairs_transformed"] and d["excluded_audited"] == d_s["excluded_audited"], (seq, d, d_s)
        # the first pass's rows exist: an audited search's audit pair is written (and, a row being whole, written once)
        for g, (p0, n_pairs, n_seg) in enumerate(geo):
            assert written[p0:p0 + n_pairs].any(), (seq, g)
            if P.audited(g, seq, every):
                assert written[p0 + P.audit_pair(g, seq, n_pairs)], (seq, g)
    return geo, got["search"]


PARAMS = [(m, t, e) for m in ("sqdiff_normed", "ccoeff_normed") for t in ("u8", "f32") for e in (1, 2)]


@pytest.mark.parametrize("method,dtype,every", PARAMS)
def test_job_a_every_count_of_pairs_to_form(lib, monkeypatch, method, dtype, every):
    """Searches with 0, 1, C, C + 1 and 2 C + 1 pairs formed behind the pilot -- found in the `search` route's written rows, not
    assumed --, none above two fifths of its pairs; patterns of 1 to 30 segments."""
    planted, mpair = _made("A", method)[6:8]
    geo, runs = _both_routes(lib, monkeypatch, "A", method, dtype, every)
    assert [s for _, _, s in geo] == A_SEGS and all(n == WINDOW for _, n, _ in geo)
    for seq, res, d, written, yw in runs:
        counts = _behind(geo, written, seq, every)
        assert {0, 1, C, C + 1, 2 * C + 1} <= set(counts), (seq, counts)
        for g, (p0, n_pairs, _) in enumerate(geo):
            assert written[p0:p0 + n_pairs].sum() * 5 <= n_pairs * 2, (seq, g)                 # (off the dense form)
            assert all(written[p0 + i] for i in planted[g]) and written[p0 + mpair[g]], (seq, g)   # the tied pairs are formed


@pytest.mark.parametrize("method,dtype,every", PARAMS)
def test_job_b_a_long_window_across_the_64_pair_steps(lib, monkeypatch, method, dtype, every):
    planted = _made("B", method)[6][0]
    assert {63, 64, 255, 256, B_PAIRS - 1} <= set(planted)
    assert all(P.audit_pair(0, seq, B_PAIRS) in planted for seq in RUNS[every])
    geo, runs = _both_routes(lib, monkeypatch, "B", method, dtype, every)
    assert geo == [(0, B_PAIRS, 1)]
    for seq, res, d, written, yw in runs:
        assert written[0] and all(written[i] for i in planted), seq
        assert written.sum() * 5 <= B_PAIRS * 2, (seq, int(written.sum()))                      # (off the dense form)


@pytest.mark.parametrize("lone", [False, True])
@pytest.mark.parametrize("method,dtype,every", PARAMS)
def test_job_c_items_next_to_the_dense_form(lib, monkeypatch, method, dtype, every, lone):
    """The searches for noise list more than two fifths of their pairs; two of them hold an eighth of the sub-batch's pairs and
    take the dense form, a lone one does not and its pairs become items (dense_repack_kernel's rule, stated on the written rows)."""
    name = "C-lone" if lone else "C"
    planted = _made(name, method)[6]
    geo, runs = _both_routes(lib, monkeypatch, name, method, dtype, every)
    total = sum(n for _, n, _ in geo)
    for seq, res, d, written, yw in runs:
        dense_listed = 0
        for g, (p0, n_pairs, _) in enumerate(geo):
            listed = int(written[p0:p0 + n_pairs].sum())
            if planted[g] is None:
                assert listed * 5 > n_pairs * 2, (seq, g, listed, n_pairs)
                dense_listed += listed
            else:
                assert listed * 5 <= n_pairs * 2, (seq, g, listed, n_pairs)
        assert (dense_listed < total // 8) == lone, (seq, dense_listed, total)
        assert max(_behind(geo[:len(A_SEGS)], written, seq, every)) > C                       # items exist beside them, more than one of a search
