"""Best-K runs (sushi_hip_batch_run_best, SearchBatch.best, sushi_amd.occurrences.find_best, WavStream.find_best_matches) on the
MI355X.

The picks of a request must be exactly best_peaks (greedy suppression on the host) of its whole curve (sushi_hip_match_curves,
itself bitwise the oracle for uint8): indices equal, score bits equal, counts equal -- whatever K, the separation, the threshold, the
exclusion's mode or form, the sub-batch cuts and the lanes; the exclusion must exclude, and be audited; argmin and threshold runs on
the same batch must not notice."""
import itertools

import numpy as np
import pytest

from sushi_amd import synth
from sushi_amd.occurrences import best_peaks

import test_occurrences_gpu as T          # its helpers: planted copies, stream rows, curves, ragged batches

pytestmark = pytest.mark.gpu

RATE = T.RATE
PAIR = T.PAIR
TILE = 1024
M3 = T.M3
_bits = T._bits


def _want(curves, lens, k, sep, method, thr):
    return [best_peaks(c, k, m if sep is None else sep, method, threshold=thr) for c, m in zip(curves, lens)]


def _assert_best(found, want, what=None):
    assert len(found) == len(want)
    for j, ((gi, gs), (wi, ws)) in enumerate(zip(found, want)):
        assert gi.dtype == np.int64 and gs.dtype == np.float32
        assert gi.tolist() == wi.tolist(), (what, j, gi.tolist(), wi.tolist())
        assert _bits(gs).tolist() == _bits(ws).tolist(), (what, j)


def _same(a, b, what=None):
    assert len(a) == len(b)
    for j, ((i0, s0), (i1, s1)) in enumerate(zip(a, b)):
        assert i0.tolist() == i1.tolist() and _bits(s0).tolist() == _bits(s1).tolist(), (what, j)


# ---- 1. planted copies: best_peaks on the curves, bitwise ------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ccoeff_normed", "sqdiff_normed"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_planted_copies_are_best_peaks_on_the_curves(dtype, method):
    places = T.PLACES                                                   # 5 copies, gains 0.35 - 1, 0 - 99 dB
    pcm, a = T._planted(60, M3, places, seed=11)
    row = T._rows(pcm, dtype)
    dst, src = T._streams(row)
    n = row.shape[0]
    # the whole stream; a window that holds three copies; a small window around one copy
    offs, lens = [a, a, a], [M3, M3, M3]
    wst, npos = [0, 150000, 329000], [n - M3 + 1, 400000, 3000]
    curves = T._curves(dst, src, offs, lens, wst, npos, method)
    peak = np.sort(np.array([curves[0][b] for b, _, _ in places], np.float32))
    cc = method == "ccoeff_normed"
    # no threshold; one between the copies' peaks; one EQUAL to a curve value (it passes); one nothing passes
    taus = [None, float((np.float64(peak[2]) + peak[3]) / 2), float(peak[1]), 1.5 if cc else -0.5]
    b = T._batch(dst, src, offs, lens, wst, npos, method)
    copies = len(places)
    for k, sep, thr in itertools.product((1, 2, copies, copies + 3, 32), (1, 100, None, 3 * PAIR), taus):
        found = b.best(k, sep, thr)
        _assert_best(found, _want(curves, lens, k, sep, method, thr), (k, sep, thr))
        if thr == taus[3]:
            assert all(i.size == 0 for i, _ in found)
        if thr == taus[2] and k >= copies and sep is None:          # (the copy whose peak IS the threshold passes it)
            assert [p for p, _, _ in places if curves[0][p] == peak[1]][0] in found[0][0]
        assert b.diagnostics()["slb_violations"] == 0
    # the copies themselves, best first
    got = b.best(copies, None)[0][0].tolist()
    order = np.argsort([-curves[0][p] if cc else curves[0][p] for p, _, _ in places], kind="stable")
    assert got == [places[j][0] for j in order]


# ---- 2. a pick's window against tiles, pairs and the window's ends ---------------------------------------------------------
@pytest.mark.parametrize("method", ["ccoeff_normed", "sqdiff_normed"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_picks_next_to_tile_pair_and_window_ends(dtype, method):
    m = 2000
    # copies at the last position of a pair, the first of one, the last of a tile, the first of one, and one mid-tile
    at = [5000, 2 * PAIR - 1, 5 * PAIR, 7 * PAIR + 3 * TILE - 1, 9 * PAIR + 5 * TILE, 12 * PAIR + 700]
    pcm, a = T._planted(40, m, [(at[0], 1, 99)] + [(p, 0.9, 20) for p in at[1:]], seed=21)
    row = T._rows(pcm, dtype)
    dst, src = T._streams(row)
    n = row.shape[0]
    offs, lens, wst, npos = [], [], [], []
    # the whole stream; windows whose first / last position is a copy; windows cut inside a pair on both sides; n_pos 1 on a copy
    for ws, p in ((0, n - m + 1), (at[2], 3 * PAIR), (at[1] - 2 * PAIR + 1, 2 * PAIR), (at[3], 1), (at[3] - 100, 2 * PAIR + 333),
                  (n - m + 1 - PAIR - 5, PAIR + 5), (at[4] - TILE, 2 * TILE + 1)):
        offs.append(a); lens.append(m); wst.append(ws); npos.append(p)
    curves = T._curves(dst, src, offs, lens, wst, npos, method)
    b = T._batch(dst, src, offs, lens, wst, npos, method)
    thr = 0.5
    # separations whose window ends fall inside the picked tile, in a neighbouring tile, in the neighbouring pair, far away
    for k, sep, t in itertools.product((1, 3, 7, 32), (1, 2, 300, TILE, 1500, PAIR - 1, PAIR, 3 * PAIR), (None, thr)):
        _assert_best(b.best(k, sep, t), _want(curves, lens, k, sep, method, t), (k, sep, t))
    assert b.diagnostics()["slb_violations"] == 0


# ---- 3. every score ties: a constant stream, a periodic one ----------------------------------------------------------------
@pytest.mark.parametrize("method", ["ccoeff_normed", "sqdiff_normed"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_constant_and_periodic_streams_tie_by_the_lower_index(dtype, method):
    n = 6 * PAIR + 1234
    const = np.full(n, 77, np.uint8) if dtype == np.uint8 else np.full(n, 0.3, np.float32)
    period = 3000
    one = synth.make_dst_pcm(period / RATE, RATE, seed=31)[:period]
    periodic = T._rows(np.tile(one, n // period + 1)[:n], dtype)
    for name, row in (("constant", const), ("periodic", periodic)):
        dst, src = T._streams(row)
        offs, lens, wst, npos = [100, 40000, 7], [1500, 5000, 900], [0, 10000, 2 * PAIR - 50], [n - 1500 + 1, 3 * PAIR, PAIR + 100]
        curves = T._curves(dst, src, offs, lens, wst, npos, method)
        for exclusion in ("always", "never"):
            b = T._batch(dst, src, offs, lens, wst, npos, method, exclusion=exclusion)
            for k, sep in ((1, None), (8, 5000), (32, PAIR), (5, 1), (32, 700), (4, period), (6, period + 1)):
                found = b.best(k, sep)
                _assert_best(found, _want(curves, lens, k, sep, method, None), (name, exclusion, k, sep))
                if name == "constant":
                    assert np.unique(_bits(curves[0])).size == 1
                    s = lens[0] if sep is None else sep
                    assert found[0][0].tolist() == list(range(0, npos[0], s))[:k]
            if name == "periodic" and dtype == np.uint8:
                # the pattern recurs exactly every period (integer sums: the very same score), the lower index first
                got = b.best(4, period)[0]
                assert got[0].tolist() == [100 % period + j * period for j in range(4)] and np.unique(_bits(got[1])).size == 1


# ---- 4. forms, cuts, lanes, ragged batches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["ccoeff_normed", "sqdiff_normed"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_every_form_and_cut_gives_the_same_picks(dtype, method):
    pcm, a = T._planted(40, M3, [(60000, 1, 99), (250000, 0.8, 10), (400000, 0.5, 3)], seed=12)
    row = T._rows(pcm, dtype)
    dst, src = T._streams(row)
    rng = np.random.default_rng(3)
    # patterns of one segment up to mac_long_kernel's lengths, windows clipped at both stream ends, n_pos of 1
    offs, lens, wst, npos = T._ragged(row.shape[0], rng, M3, a)
    curves = T._curves(dst, src, offs, lens, wst, npos, method)
    t = 0.45 if method == "ccoeff_normed" else 0.6
    asks = [(3, None, None), (2, 100, t), (32, 3 * PAIR, None), (1, 1, None)]
    ref = None
    for form in ("never", "always", "band", "whole", "auto"):
        b = T._batch(dst, src, offs, lens, wst, npos, method, exclusion=form)
        got = [b.best(*ask) for ask in asks]
        if ref is None:
            for ask, g in zip(asks, got):
                _assert_best(g, _want(curves, lens, ask[0], ask[1], method, ask[2]), ask)
            assert b.diagnostics()["pairs_transformed"] == b.fft_pairs
            ref = got
        else:
            for ask, r, g in zip(asks, ref, got):
                _same(r, g, (form, ask))
        assert b.diagnostics()["slb_violations"] == 0
    # several sub-batches (a workspace that holds about one search)
    small = T._batch(dst, src, offs, lens, wst, npos, method, workspace_bytes=4 << 20)
    assert small.sub_batches > 3
    for ask, r in zip(asks, ref):
        _same(r, small.best(*ask), ("4 MB", ask))


def test_a_lanes_sized_batch_gives_the_same_picks_on_any_lanes(monkeypatch):
    """128 searches and >= 24 k block pairs: the size at which the library runs a batch on lanes by itself."""
    n = 210 * PAIR
    pcm, a = T._planted(n / RATE, 2000, [(100000, 1, 99), (2000000, 0.9, 12), (4000000, 0.7, 6)], seed=13)
    row = T._rows(pcm, np.uint8)
    dst, src = T._streams(row)
    rng = np.random.default_rng(4)
    offs = [a] * 32 + [int(x) for x in rng.integers(0, n - 3000, 96)]
    lens = [2000] * 32 + [int(x) for x in rng.integers(900, 3000, 96)]
    wst = [int(x) for x in rng.integers(0, 6 * PAIR, 128)]
    npos = [n - w - m + 1 - int(rng.integers(0, PAIR)) for w, m in zip(wst, lens)]
    method = "ccoeff_normed"
    asks = [(3, None, 0.6), (2, 500, None)]
    outs, infos = [], []
    for lanes in ("1:1", "2:2", "4:2", None):
        if lanes is None:
            monkeypatch.delenv("SUSHI_HIP_LANES", raising=False)
        else:
            monkeypatch.setenv("SUSHI_HIP_LANES", lanes)
        b = T._batch(dst, src, offs, lens, wst, npos, method)
        outs.append([b.best(*ask) for ask in asks])
        infos.append((b.lanes, b.sub_batches, b.fft_pairs))
        assert b.diagnostics()["slb_violations"] == 0
    assert infos[0][2] >= 24 * 1024 and infos[0][:2] == (1, 1) and infos[1][0] == 2 and infos[-1][0] >= 2, infos
    for o in outs[1:]:
        for ask, r, g in zip(asks, outs[0], o):
            _same(r, g, ask)
    pick = [0, 1, 40, 127]
    curves = T._curves(dst, src, [offs[k] for k in pick], [lens[k] for k in pick], [wst[k] for k in pick], [npos[k] for k in pick], method)
    for ask, out in zip(asks, outs[0]):
        _assert_best([out[k] for k in pick], _want(curves, [lens[k] for k in pick], ask[0], ask[1], method, ask[2]), ask)
    assert outs[0][0][0][0].size == 3


# ---- 5. K = 1 is the argmin run; other runs on the same batch do not notice -------------------------------------------------
def test_best_runs_interleaved_with_runs_and_threshold_runs_change_none():
    pcm, a = T._planted(45, M3, [(40000, 1, 99), (200000, 0.9, 12), (420000, 0.7, 6)], seed=16)
    row = T._rows(pcm, np.uint8)
    dst, src = T._streams(row)
    n = row.shape[0]
    rng = np.random.default_rng(16)
    offs = [a] + [int(x) for x in rng.integers(0, n - M3, 5)]
    k = len(offs)
    lens = [M3] * k
    wst = [0] + [int(x) for x in rng.integers(0, n // 2, 5)]
    npos = [n - M3 + 1] + [int(x) for x in rng.integers(PAIR, n // 2 - M3, 5)]
    b = T._batch(dst, src, offs, lens, wst, npos, "sqdiff_normed", exclusion="auto")

    def check_run(method, curves):
        idx, score = b.run()
        idx, score = idx.cpu().numpy(), score.cpu().numpy()
        for j, c in enumerate(curves):
            e = int(np.argmax(c) if method == "ccoeff_normed" else np.argmin(c))
            assert idx[j] == e and _bits(score[j]) == _bits(c[e]), (method, j)
        return idx, score

    def check_best(method, curves, idx, score):
        one = b.best(1)
        for j, (bi, bs) in enumerate(one):
            assert bi.tolist() == [int(idx[j])] and _bits(bs).tolist() == [int(_bits(score[j]))], (method, j)
        _assert_best(b.best(3, 2000), _want(curves, lens, 3, 2000, method, None), method)

    def check_threshold(method, curves, t):
        T._assert_hits_are_the_curves(b.occurrences(t), curves, t, method)

    c_sq = T._curves(dst, src, offs, lens, wst, npos, "sqdiff_normed")
    idx, score = check_run("sqdiff_normed", c_sq)
    check_best("sqdiff_normed", c_sq, idx, score)
    idx, score = check_run("sqdiff_normed", c_sq)
    check_threshold("sqdiff_normed", c_sq, 0.9)
    check_best("sqdiff_normed", c_sq, idx, score)
    check_threshold("sqdiff_normed", c_sq, 0.9)
    b.set_method("ccoeff_normed")
    c_cc = T._curves(dst, src, offs, lens, wst, npos, "ccoeff_normed")
    _assert_best(b.best(2), _want(c_cc, lens, 2, None, "ccoeff_normed", None))      # (before the method's first run: the form is decided here)
    idx, score = check_run("ccoeff_normed", c_cc)
    check_best("ccoeff_normed", c_cc, idx, score)
    check_threshold("ccoeff_normed", c_cc, 0.3)
    idx, score = check_run("ccoeff_normed", c_cc)
    offs2 = offs[::-1]
    assert b.reset(offs2, lens, wst, npos)
    c_2 = T._curves(dst, src, offs2, lens, wst, npos, "ccoeff_normed")
    _assert_best(b.best(3, None, 0.5), _want(c_2, lens, 3, None, "ccoeff_normed", 0.5))
    idx, score = check_run("ccoeff_normed", c_2)
    check_best("ccoeff_normed", c_2, idx, score)
    idx, score = check_run("ccoeff_normed", c_2)


# ---- 6. the exclusion excludes, and is audited -----------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_the_exclusion_works_and_is_audited(dtype):
    """Every request has exactly K strong copies.  The bar: the best-K run evaluates no more pairs than a threshold run at the worst
    score it returned, plus its seed pairs, plus the audit's.  The allowance follows from the seed rule (sushi_fft_best.inc): the K + 2
    pairs of smallest bound per search are evaluated before any score is known; every later pair is listed by the threshold run's
    own test (its bound against the search's K-th score, which is no worse than the batch's worst) or by the audit."""
    K, n_req = 3, 8
    seconds = 600
    n_pcm = seconds * RATE
    rng = np.random.default_rng(41)
    pcm = synth.make_dst_pcm(seconds, RATE, seed=41).astype(np.float64)
    seg = n_pcm // (n_req * K + 1)
    offs = []
    for j in range(n_req):
        a = (j * K) * seg + 1000 + 7 * j
        pat = pcm[a:a + M3].copy()
        offs.append(a)
        for c, snr in zip(range(1, K), (30.0, 20.0)):                   # gain 1, >= 20 dB
            at = (j * K + c) * seg + 1000 + 131 * c
            pcm[at:at + M3] = pat + rng.standard_normal(M3) * np.sqrt(np.mean(pat ** 2) / 10.0 ** (snr / 10.0))
    row = T._rows(np.clip(np.round(pcm), -32768, 32767).astype(np.int16), dtype)
    dst, src = T._streams(row)
    n = row.shape[0]
    lens, wst, npos = [M3] * n_req, [0] * n_req, [n - M3 + 1] * n_req
    method = "ccoeff_normed"
    b = T._batch(dst, src, offs, lens, wst, npos, method, exclusion="always")
    found = b.best(K)
    d = b.diagnostics()
    assert all(i.size == K for i, _ in found)
    worst = float(min(float(s.min()) for _, s in found))
    # the precondition on the material, from the threshold run alone: no request has hits in more than K + 2 pairs
    hits = b.occurrences(worst)
    dt = b.diagnostics()
    assert all(np.unique(i // PAIR).size <= K + 2 for i, _ in hits), [np.unique(i // PAIR).size for i, _ in hits]
    print("best-%d: %d of %d pairs evaluated exactly (threshold run at %.4f: %d), %d excluded pairs audited, band %d" %
          (K, d["pairs_transformed"], b.fft_pairs, worst, dt["pairs_transformed"], d["excluded_audited"], d["band"]))
    assert d["pairs_transformed"] <= dt["pairs_transformed"] + (K + 2) * n_req + d["excluded_audited"], (d, dt)
    assert d["slb_violations"] == 0 and d["excluded_audited"] > 0, d
    assert d["flagged"] == 0 and d["tiles_dense"] == 0 and d["suspended"] == 0 and d["band_votes"] == [0, 0]
    curves = T._curves(dst, src, offs[:2], lens[:2], wst[:2], npos[:2], method)
    _assert_best(found[:2], _want(curves, lens[:2], K, None, method, None))
    for j, (i, _) in enumerate(found):
        assert i[0] == offs[j]


def test_a_direct_path_batch_is_refused():
    import torch
    from sushi_amd import _native
    from sushi_amd.common import SushiError
    from sushi_amd.device import SearchBatch
    row = T._rows(synth.make_dst_pcm(5, RATE, seed=17), np.uint8)
    dst, src = T._streams(row)
    b = SearchBatch(dst, src, [100], [1000], [0], [5000], path="direct")
    with pytest.raises(SushiError):
        b.run_best(2)
    hits = torch.empty(16, dtype=torch.int32, device=dst.device)
    counts = torch.empty(2, dtype=torch.int32, device=dst.device)
    assert _native.lib().sushi_hip_batch_run_best(b.handle, 2, 0, None, hits.data_ptr(), counts.data_ptr(), None) == -1
    f = SearchBatch(dst, src, [100], [1000], [0], [5000], path="fft")
    assert _native.lib().sushi_hip_batch_run_best(f.handle, 2, 0, None, hits.data_ptr() + 2, counts.data_ptr(), None) == -2
    with pytest.raises(SushiError):
        f.run_best(0)
    with pytest.raises(SushiError):
        f.run_best(33)
    with pytest.raises(SushiError):
        f.run_best(2, min_separation=0)
    with pytest.raises(SushiError):
        f.run_best(2, threshold=float("nan"))


# ---- 7. find_best, WavStream.find_best_matches -----------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_find_best_matches(tmp_path, sample_type):
    from sushi_amd.occurrences import find_best
    from sushi_amd.wav import WavStream
    seconds = 80
    places = [(int(s * RATE), g, snr) for s, g, snr in ((7.5, 1.0, 99), (21.25, 0.9, 20), (40.0, 0.8, 12), (66.5, 0.7, 9))]
    src_pcm = synth.make_dst_pcm(10, RATE, seed=19)
    dst_pcm = synth.make_dst_pcm(seconds, RATE, seed=18).astype(np.float64)
    pat = src_pcm[2 * RATE:2 * RATE + M3].astype(np.float64)
    rng = np.random.default_rng(18)
    for at, g, snr in places:
        noise = rng.standard_normal(M3) * np.sqrt(np.mean(pat ** 2) / 10.0 ** (snr / 10.0))
        dst_pcm[at:at + M3] = g * pat + noise
    synth.write_wav(str(tmp_path / "dst.wav"), np.clip(np.round(dst_pcm), -32768, 32767).astype(np.int16), RATE)
    synth.write_wav(str(tmp_path / "src.wav"), src_pcm, RATE)
    dws = WavStream(str(tmp_path / "dst.wav"), sample_type=sample_type)
    sws = WavStream(str(tmp_path / "src.wav"), sample_type=sample_type)
    pattern = sws.get_substream(2.0, 5.0)
    scores, times = dws.find_best_matches(pattern, len(places))
    assert scores.dtype == np.float32 and len(times) == scores.size == len(places)
    assert np.all(np.diff(scores) <= 0)                                 # best first
    assert sorted(round(t * RATE) for t in times) == sorted(at for at, _, _ in places) or \
        all(np.min(np.abs(np.asarray(times) - at / RATE)) < 1.5 / RATE for at, _, _ in places)
    # the picks are what thinning all hits gives (find_occurrences with the same separation), best first
    ps, pt = dws.find_occurrences(pattern, float(scores.min()), min_separation=3.0)
    assert sorted(_bits(ps).tolist()) == sorted(_bits(scores).tolist()) and sorted(pt) == sorted(times)
    # the best one is find_substream's answer
    d, tt = dws.find_substreams([pattern], [dws.duration_seconds / 2.0], [dws.duration_seconds / 2.0 + dws.PADDING_SECONDS],
                                method="ccoeff_normed")
    assert _bits(d[0]) == _bits(scores[0]) and abs(tt[0] - times[0]) < 1.01 / RATE
    # a threshold cuts the list short; a window around one copy holds one
    s2, t2 = dws.find_best_matches(pattern, 32, threshold=0.5, min_separation=1.0)
    assert len(t2) == len(places) and _bits(s2).tolist() == _bits(scores).tolist()
    many = dws.find_best_matches_many([pattern, pattern], 3, [None, 40.0], [None, 5.0], threshold=0.5)
    assert _bits(many[0][0]).tolist() == _bits(scores[:3]).tolist() and many[0][1] == times[:3]
    assert len(many[1][1]) == 1 and abs(many[1][1][0] - 40.0) < 1.5 / RATE
    # the array form on the streams themselves
    D, S = dws.device_stream(), dws.device_stream()
    at = places[0][0] + int(round(dws.padding_size))
    got = find_best(D, S, [at], [M3], [0], [D.n - M3 + 1], 2, method="ccoeff_normed")
    assert got[0][0][0] == at and got[0][1][0] > 0.9999                 # (the stretch against itself)
