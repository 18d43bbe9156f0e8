"""Threshold runs (sushi_hip_batch_run_threshold, SearchBatch.occurrences, sushi_amd.occurrences, WavStream.find_occurrences) on
the MI355X.

The hits of a request must be exactly np.where on its whole curve (sushi_hip_match_curves, itself bitwise the oracle for uint8),
with bitwise scores, whatever the exclusion's mode or form, the sub-batch cuts and the lanes; the exclusion must exclude, and be
audited; argmin runs on the same batch must not notice."""
import numpy as np
import pytest

from sushi_amd import synth

pytestmark = pytest.mark.gpu

RATE = 12000
PAIR = 24576                   # positions of a block pair (2 FFT_H)


def _rows(pcm, dtype):
    """int16 PCM -> a stream row as WavStream.data holds it (min/max scaled to [0, 1]; uint8: x 255 + 0.5 truncated)."""
    x = pcm.astype(np.float64)
    x = ((x - x.min()) / (x.max() - x.min())).astype(np.float32)
    return (x * np.float32(255.0) + np.float32(0.5)).astype(np.uint8) if dtype == np.uint8 else x


def _planted(seconds, m, places, seed):
    """An audio-like stream with copies of one of its own stretches planted at `places` [(sample, gain, snr_db)]: returns the
    int16 PCM and where the pattern is (the first copy, exact)."""
    rng = np.random.default_rng(seed)
    pcm = synth.make_dst_pcm(seconds, RATE, seed=seed).astype(np.float64)
    a = places[0][0]
    pat = pcm[a:a + m].copy()
    p_sig = float(np.mean(pat ** 2))
    for b, gain, snr in places[1:]:
        noise = rng.standard_normal(m) * np.sqrt(p_sig / 10.0 ** (snr / 10.0))
        pcm[b:b + m] = gain * pat + noise
    return np.clip(np.round(pcm), -32768, 32767).astype(np.int16), a


def _streams(row):
    from sushi_amd.device import DeviceStream
    s = DeviceStream(row)
    return s, s


def _curves(dst, src, offs, lens, wst, npos, method):
    from sushi_amd.curves import match_curves
    c, o = match_curves(dst, src, offs, lens, wst, npos, method=method)
    c = c.cpu().numpy()
    return [c[o[k]:o[k + 1]] for k in range(len(offs))]


def _where(curve, t, method):
    return np.flatnonzero(curve >= np.float64(t)) if method == "ccoeff_normed" else np.flatnonzero(curve <= np.float64(t))


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _batch(dst, src, offs, lens, wst, npos, method, exclusion="always", workspace_bytes=None):
    from sushi_amd.device import SearchBatch
    return SearchBatch(dst, src, offs, lens, wst, npos, path="fft", method=method, exclusion=exclusion,
                       workspace_bytes=workspace_bytes)


def _assert_hits_are_the_curves(found, curves, t, method):
    for k, ((idx, sc), curve) in enumerate(zip(found, curves)):
        want = _where(curve, t, method)
        assert idx.dtype == np.int64 and sc.dtype == np.float32
        assert np.array_equal(idx, want), (k, t, idx.size, want.size, np.setxor1d(idx, want)[:8])
        assert np.array_equal(_bits(sc), _bits(curve[want])), k


def _same(a, b):
    assert len(a) == len(b)
    for (i0, s0), (i1, s1) in zip(a, b):
        assert np.array_equal(i0, i1) and np.array_equal(_bits(s0), _bits(s1))


# ---- 1. planted occurrences: np.where on the curves, bitwise; uint8 against the oracle too -------------------------------
M3 = 3 * RATE
PLACES = [(50000, 1.0, 99.0), (200000, 0.9, 20.0), (330000, 0.6, 6.0), (470000, 0.35, 0.0), (600000, 0.8, 12.0)]


@pytest.mark.parametrize("method", ["ccoeff_normed", "sqdiff_normed"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_planted_occurrences_are_where_on_the_curves(oracle, dtype, method):
    pcm, a = _planted(60, M3, PLACES, seed=11)
    row = _rows(pcm, dtype)
    dst, src = _streams(row)
    n = row.shape[0]
    # the whole stream; a window that holds three copies; a small window around one copy (the oracle's size)
    offs = [a, a, a]
    lens = [M3, M3, M3]
    wst = [0, 150000, 329000]
    npos = [n - M3 + 1, 400000, 3000]
    curves = _curves(dst, src, offs, lens, wst, npos, method)
    whole = curves[0]
    peak = np.array([whole[b] for b, _, _ in PLACES], np.float32)
    # thresholds between the planted copies' peaks, and one EQUAL to a curve value (inclusive comparison)
    srt = np.sort(peak)
    taus = [float(srt[1]), float((np.float64(srt[2]) + srt[3]) / 2), float(srt[0]) * (1.0001 if method == "sqdiff_normed" else 0.9999)]
    b = _batch(dst, src, offs, lens, wst, npos, method)
    for t in taus:
        found = b.occurrences(t)
        _assert_hits_are_the_curves(found, curves, t, method)
        # (the exact curve value is a hit)
        if t == float(srt[1]):
            j = int(np.flatnonzero(peak == srt[1])[0])
            assert PLACES[j][0] in found[0][0]
        d = b.diagnostics()
        assert d["slb_violations"] == 0 and d["flagged"] == 0 and d["candidates"] == 0, d
    if dtype == np.uint8:
        w, p = wst[2], npos[2]
        ref = oracle.match_template_direct(row[w:w + p + M3 - 1], row[a:a + M3], method=method)[0]
        assert np.array_equal(_bits(ref), _bits(curves[2]))
        t = taus[0]
        found = b.occurrences(t)
        assert np.array_equal(found[2][0], _where(ref, t, method)) and np.array_equal(_bits(found[2][1]), _bits(ref[found[2][0]]))


# ---- 2. forms, cuts, lanes, ragged batches ---------------------------------------------------------------------------------
def _ragged(n, rng, m_pat, a):
    """patterns of 1 segment up to mac_long_kernel's lengths, windows clipped at both ends, n_pos of 1"""
    offs, lens, wst, npos = [], [], [], []
    for m in (500, 4096, m_pat, 40000, 80000, 100000):
        o = a if m == m_pat else int(rng.integers(0, n - m))
        for ws, p in ((0, 3 * PAIR + 77), (n - m + 1 - 2 * PAIR, 2 * PAIR), (int(rng.integers(0, n - m - PAIR)), 1),
                      (0, n - m + 1)):
            offs.append(o); lens.append(m); wst.append(ws); npos.append(p)
    return offs, lens, wst, npos


@pytest.mark.parametrize("method", ["ccoeff_normed", "sqdiff_normed"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_every_form_and_cut_gives_the_same_hits(dtype, method):
    pcm, a = _planted(40, M3, [(60000, 1, 99), (250000, 0.8, 10), (400000, 0.5, 3)], seed=12)
    row = _rows(pcm, dtype)
    dst, src = _streams(row)
    rng = np.random.default_rng(3)
    offs, lens, wst, npos = _ragged(row.shape[0], rng, M3, a)
    curves = _curves(dst, src, offs, lens, wst, npos, method)
    t = 0.45 if method == "ccoeff_normed" else 0.6
    ref = None
    for form in ("never", "always", "band", "whole", "auto"):
        b = _batch(dst, src, offs, lens, wst, npos, method, exclusion=form)
        got = b.occurrences(t)
        if ref is None:
            _assert_hits_are_the_curves(got, curves, t, method)
            assert b.diagnostics()["pairs_transformed"] == b.fft_pairs
            ref = got
        else:
            _same(ref, got)
        assert b.diagnostics()["slb_violations"] == 0
    # several sub-batches (a workspace that holds about one search)
    small = _batch(dst, src, offs, lens, wst, npos, method, workspace_bytes=4 << 20)
    assert small.sub_batches > 3
    _same(ref, small.occurrences(t))


def test_a_lanes_sized_batch_gives_the_same_hits_on_any_lanes(monkeypatch):
    """128 searches and >= 24 k block pairs: the size at which the library runs a batch on lanes by itself."""
    n = 210 * PAIR
    pcm, a = _planted(n / RATE, 2000, [(100000, 1, 99), (2000000, 0.9, 12), (4000000, 0.7, 6)], seed=13)
    row = _rows(pcm, np.uint8)
    dst, src = _streams(row)
    rng = np.random.default_rng(4)
    offs = [a] * 32 + [int(x) for x in rng.integers(0, n - 3000, 96)]
    lens = [2000] * 32 + [int(x) for x in rng.integers(900, 3000, 96)]
    wst = [int(x) for x in rng.integers(0, 6 * PAIR, 128)]
    npos = [n - w - m + 1 - int(rng.integers(0, PAIR)) for w, m in zip(wst, lens)]
    method, t = "ccoeff_normed", 0.6
    outs, infos = [], []
    for lanes in ("1:1", "2:2", "4:2", None):
        if lanes is None:
            monkeypatch.delenv("SUSHI_HIP_LANES", raising=False)
        else:
            monkeypatch.setenv("SUSHI_HIP_LANES", lanes)
        b = _batch(dst, src, offs, lens, wst, npos, method)
        outs.append(b.occurrences(t))
        infos.append((b.lanes, b.sub_batches, b.fft_pairs))
        assert b.diagnostics()["slb_violations"] == 0
    assert infos[0][2] >= 24 * 1024 and infos[0][:2] == (1, 1) and infos[1][0] == 2 and infos[-1][0] >= 2, infos
    for o in outs[1:]:
        _same(outs[0], o)
    pick = [0, 1, 40, 127]
    curves = _curves(dst, src, [offs[k] for k in pick], [lens[k] for k in pick], [wst[k] for k in pick], [npos[k] for k in pick], method)
    _assert_hits_are_the_curves([outs[0][k] for k in pick], curves, t, method)
    assert outs[0][0][0].size > 0


# ---- 3. capacity -----------------------------------------------------------------------------------------------------------
def test_counts_are_exact_beyond_the_capacity_and_occurrences_retries_once():
    pcm, a = _planted(30, M3, [(30000, 1, 99), (150000, 0.9, 20), (250000, 0.8, 10)], seed=14)
    row = _rows(pcm, np.uint8)
    dst, src = _streams(row)
    n = row.shape[0]
    offs, lens, wst, npos = [a, a, 7], [M3, M3, 5000], [0, 100000, 0], [n - M3 + 1, 60000, n - 5000 + 1]
    method, t = "ccoeff_normed", 0.2
    curves = _curves(dst, src, offs, lens, wst, npos, method)
    want = [_where(c, t, method) for c in curves]
    assert all(w.size > 2 for w in want)
    b = _batch(dst, src, offs, lens, wst, npos, method)
    for cap in (0, 1, int(want[0].size // 2)):
        hits, counts = b.run_threshold(t, cap)
        counts = counts.cpu().numpy()
        assert counts.tolist() == [w.size for w in want]
        h = hits.cpu().numpy()
        assert h.shape == (3, cap, 2)
        for k in range(3):
            m = min(cap, want[k].size)
            assert np.array_equal(h[k, :m, 0], want[k][:m])
            assert np.array_equal(h[k, :m, 1].view(np.uint32), _bits(curves[k][want[k][:m]]))
    found = b.occurrences(t, capacity=8)
    _assert_hits_are_the_curves(found, curves, t, method)


# ---- 4. the exclusion excludes, and is audited ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_the_exclusion_works_and_is_audited(dtype):
    seconds = 600
    rng = np.random.default_rng(15)
    places = [(int(x), float(g), float(s)) for x, g, s in zip(rng.integers(0, seconds * RATE - M3, 6) // 7 * 7,
                                                               (1.0, 0.9, 0.8, 0.7, 0.9, 0.6), (99, 20, 12, 9, 6, 15))]
    pcm, a = _planted(seconds, M3, places, seed=15)
    row = _rows(pcm, dtype)
    dst, src = _streams(row)
    n = row.shape[0]
    offs = [a] + [int(x) for x in rng.integers(0, n - M3, 7)]
    k = len(offs)
    b = _batch(dst, src, offs, [M3] * k, [0] * k, [n - M3 + 1] * k, "ccoeff_normed")
    found = b.occurrences(0.8)
    d = b.diagnostics()
    print("threshold 0.8: %d of %d pairs evaluated exactly, %d excluded pairs audited, band %d" %
          (d["pairs_transformed"], b.fft_pairs, d["excluded_audited"], d["band"]))
    # (the bar: measured 22 of 2,336 pairs on this material at 0.8, band-split form; kept well below 100 %)
    assert d["pairs_transformed"] <= 0.05 * b.fft_pairs, d
    assert d["excluded_audited"] > 0 and d["slb_violations"] == 0 and 0.0 < d["max_slb_ratio_excluded"] < 1.0, d
    assert d["flagged"] == 0 and d["tiles_dense"] == 0 and d["suspended"] == 0 and d["band_votes"] == [0, 0]
    assert found[0][0].size > 0
    curve = _curves(dst, src, offs[:1], [M3], [0], [n - M3 + 1], "ccoeff_normed")
    _assert_hits_are_the_curves(found[:1], curve, 0.8, "ccoeff_normed")


# ---- 5. argmin runs on the same batch do not notice -------------------------------------------------------------------------
def test_threshold_runs_interleaved_with_runs_change_no_run():
    pcm, a = _planted(45, M3, [(40000, 1, 99), (200000, 0.9, 12), (420000, 0.7, 6)], seed=16)
    row = _rows(pcm, np.uint8)
    dst, src = _streams(row)
    n = row.shape[0]
    rng = np.random.default_rng(16)
    offs = [a] + [int(x) for x in rng.integers(0, n - M3, 5)]
    k = len(offs)
    wst = [0] + [int(x) for x in rng.integers(0, n // 2, 5)]
    npos = [n - M3 + 1] + [int(x) for x in rng.integers(PAIR, n // 2 - M3, 5)]
    b = _batch(dst, src, offs, [M3] * k, wst, npos, "sqdiff_normed", exclusion="auto")

    def check_run(method, offs_, wst_, npos_):
        idx, score = b.run()
        idx, score = idx.cpu().numpy(), score.cpu().numpy()
        curves = _curves(dst, src, offs_, [M3] * k, wst_, npos_, method)
        for j, c in enumerate(curves):
            e = int(np.argmax(c) if method == "ccoeff_normed" else np.argmin(c))
            assert idx[j] == e and _bits(score[j]) == _bits(c[e]), (method, j)
        return idx, score

    def check_threshold(method, t, idx, score):
        found = b.occurrences(t)
        for j, (hi, hs) in enumerate(found):
            passes = score[j] >= t if method == "ccoeff_normed" else score[j] <= t
            if passes:
                pos = np.searchsorted(hi, idx[j])
                assert pos < hi.size and hi[pos] == idx[j] and _bits(hs[pos]) == _bits(score[j])

    idx, score = check_run("sqdiff_normed", offs, wst, npos)
    check_threshold("sqdiff_normed", 0.9, idx, score)
    idx, score = check_run("sqdiff_normed", offs, wst, npos)
    check_threshold("sqdiff_normed", float(score.max()) + 1e-3, idx, score)
    b.set_method("ccoeff_normed")
    check_threshold("ccoeff_normed", 0.3, idx, score)             # (before the method's first run: the form is decided here)
    idx, score = check_run("ccoeff_normed", offs, wst, npos)
    check_threshold("ccoeff_normed", float(score.min()) - 1e-3, idx, score)
    offs2 = offs[::-1]
    assert b.reset(offs2, [M3] * k, wst, npos)
    _assert_hits_are_the_curves(b.occurrences(0.5), _curves(dst, src, offs2, [M3] * k, wst, npos, "ccoeff_normed"), 0.5,
                                "ccoeff_normed")
    idx, score = check_run("ccoeff_normed", offs2, wst, npos)
    check_threshold("ccoeff_normed", 0.5, idx, score)
    idx, score = check_run("ccoeff_normed", offs2, wst, npos)


def test_a_direct_path_batch_is_refused():
    from sushi_amd.common import SushiError
    from sushi_amd.device import SearchBatch
    from sushi_amd import _native
    row = _rows(synth.make_dst_pcm(5, RATE, seed=17), np.uint8)
    dst, src = _streams(row)
    b = SearchBatch(dst, src, [100], [1000], [0], [5000], path="direct")
    with pytest.raises(SushiError):
        b.run_threshold(0.5, 4)
    import torch
    hits = torch.empty(16, dtype=torch.int32, device=dst.device)
    counts = torch.empty(2, dtype=torch.int64, device=dst.device)
    assert _native.lib().sushi_hip_batch_run_threshold(b.handle, 0.5, 4, hits.data_ptr(), counts.data_ptr(), None) == -1


# ---- 6. WavStream.find_occurrences ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_find_occurrences(tmp_path, sample_type):
    from sushi_amd.wav import WavStream
    seconds = 80
    places = [(int(s * RATE), g, snr) for s, g, snr in ((7.5, 1.0, 99), (21.25, 0.9, 20), (40.0, 0.8, 12), (66.5, 0.7, 9))]
    src_pcm = synth.make_dst_pcm(10, RATE, seed=19)
    dst_pcm = synth.make_dst_pcm(seconds, RATE, seed=18).astype(np.float64)
    pat = src_pcm[2 * RATE:2 * RATE + M3].astype(np.float64)
    rng = np.random.default_rng(18)
    for b, g, snr in places:
        noise = rng.standard_normal(M3) * np.sqrt(np.mean(pat ** 2) / 10.0 ** (snr / 10.0))
        dst_pcm[b:b + M3] = g * pat + noise
    synth.write_wav(str(tmp_path / "dst.wav"), np.clip(np.round(dst_pcm), -32768, 32767).astype(np.int16), RATE)
    synth.write_wav(str(tmp_path / "src.wav"), src_pcm, RATE)
    dws = WavStream(str(tmp_path / "dst.wav"), sample_type=sample_type)
    sws = WavStream(str(tmp_path / "src.wav"), sample_type=sample_type)
    pattern = sws.get_substream(2.0, 5.0)
    scores, times = dws.find_occurrences(pattern, 0.5)
    assert scores.dtype == np.float32 and len(times) == scores.size > 0 and times == sorted(times)
    for b, _, _ in places:
        assert np.min(np.abs(np.asarray(times) - b / RATE)) < 1.5 / RATE, b
    # one peak per copy
    ps, pt = dws.find_occurrences(pattern, 0.5, min_separation=1.0)
    assert len(pt) == len(places) and ps.size == len(places)
    assert all(abs(t - b / RATE) < 1.5 / RATE for t, (b, _, _) in zip(pt, places))
    # find_substream over a window around only that peak: the same score, the same time (to find_substream's own arithmetic:
    # its start_time lies off the sample grid by less than a sample -- wav.py:178-188)
    for s, t in zip(ps, pt):
        d, tt = dws.find_substreams([pattern], [t], [2.0 / RATE], method="ccoeff_normed")
        assert _bits(d[0]) == _bits(s) and abs(tt[0] - t) < 1.01 / RATE, (t, tt, s, d)
    # the batched form, with a window given for one of them
    many = dws.find_occurrences_many([pattern, pattern], 0.5, [None, 40.0], [None, 5.0], min_separation=1.0)
    assert _bits(many[0][0]).tolist() == _bits(ps).tolist() and many[0][1] == pt
    assert len(many[1][1]) == 1 and abs(many[1][1][0] - 40.0) < 1.5 / RATE
