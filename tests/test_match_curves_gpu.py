"""Whole score curves (sushi_hip_match_curves, sushi_amd.curves, WavStream.match_template) on the MI355X.

Every value of a curve is the one the exact stages of a search compute at that position: bitwise against the oracle's
direct evaluation for uint8, bitwise against a NumPy restatement of the canonical float64 chain for float32, and the
search path's (index, score) is the first extremum of the curve and its value."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLT_EPSILON = float(np.finfo(np.float32).eps)
DBL_EPSILON = float(np.finfo(np.float64).eps)
XM = 512


def _streams(dst_row, src_row):
    from sushi_amd.device import DeviceStream
    return DeviceStream(dst_row), DeviceStream(src_row)


def _curves(dst, src, offs, lens, wst, npos, method="sqdiff_normed"):
    from sushi_amd.curves import match_curves
    c, o = match_curves(dst, src, offs, lens, wst, npos, method=method)
    c = c.cpu().numpy()
    return [c[o[k]:o[k + 1]] for k in range(len(offs))]


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _first_extremum(curve, method):
    return int(np.argmax(curve)) if method == "ccoeff_normed" else int(np.argmin(curve))


# ---- a NumPy restatement of the canonical chain and of cv2's finish (sushi_common.hpp) ---------------------------------
def _canonical_corr(t, w, pos):
    """sum T*I at positions `pos` of window row w: XM-sample chunks, each a sequential float64 sum (np.cumsum) of exact
    products, the chunk sums added in order."""
    M = t.shape[0]
    nch = (M + XM - 1) // XM
    tp = np.zeros(nch * XM, np.float64)
    tp[:M] = t
    out = np.empty(len(pos), np.float64)
    for a in range(0, len(pos), 64):
        ps = np.asarray(pos[a:a + 64], np.int64)
        win = np.zeros((ps.shape[0], nch * XM), np.float64)
        win[:, :M] = w[ps[:, None] + np.arange(M)[None, :]]
        prod = (win * tp[None, :]).reshape(ps.shape[0], nch, XM)
        cs = np.cumsum(prod, axis=2)[:, :, -1]
        tot = np.zeros(ps.shape[0], np.float64)
        for c in range(nch):
            tot = tot + cs[:, c]
        out[a:a + 64] = tot
    return out


def _finish(corr, s1, s2, t_off, w_off, pos, M, method):
    """finish_sqdiff_normed / finish_ccoeff_normed of templ_stats, in float64 (s1, s2: the streams' prefix sums)."""
    ts1, ts2 = s1["src"], s2["src"]
    tS1 = ts1[t_off + M] - ts1[t_off]
    t_sq = ts2[t_off + M] - ts2[t_off]
    inv = 1.0 / M
    t_mean = tS1 * inv
    t_var = max(t_sq * inv - t_mean * t_mean, 0.0)
    t_sdv = np.sqrt(t_var)
    t_norm2 = t_sdv * t_sdv + t_mean * t_mean
    tU = t_norm2 / inv
    tnorm = np.sqrt(t_norm2) / np.sqrt(inv)
    pos = np.asarray(pos, np.int64) + w_off
    w1, w2 = s1["dst"], s2["dst"]
    wS1 = w1[pos + M] - w1[pos]
    wU = w2[pos + M] - w2[pos]
    num = np.asarray(corr, np.float64).astype(np.float32).astype(np.float64)
    lim = np.minimum(10.0 * FLT_EPSILON * wU, 0.5)
    with np.errstate(divide="ignore", invalid="ignore"):
        if method == "sqdiff_normed":
            num = (wU - 2.0 * num) + tU
            num = np.where(num > 0.0, num, 0.0)
            diff2 = np.where(wU > 0.0, wU, 0.0)
            t = np.where(diff2 <= lim, 0.0, np.sqrt(diff2) * tnorm)
            r = np.where(num < t, num / t, 1.0)
            return r.astype(np.float32)
        if t_sdv * t_sdv < DBL_EPSILON:
            return np.ones(pos.shape[0], np.float32)
        tnorm_c = np.sqrt(t_sdv * t_sdv) / np.sqrt(inv)
        num = num - wS1 * t_mean
        diff2 = wU - (wS1 * wS1) * inv
        diff2 = np.where(diff2 > 0.0, diff2, 0.0)
        t = np.where(diff2 <= lim, 0.0, np.sqrt(diff2) * tnorm_c)
        a = np.abs(num)
        r = np.where(a < t, num / t, np.where(a < t * 1.125, np.where(num > 0.0, 1.0, -1.0), 0.0))
        return r.astype(np.float32)


def _prefix(dst, src):
    return ({"dst": dst.s1.cpu().numpy(), "src": src.s1.cpu().numpy()},
            {"dst": dst.s2.cpu().numpy(), "src": src.s2.cpu().numpy()})


def _rows(rng, dtype, n_dst, n_src):
    if dtype == np.uint8:
        return rng.integers(0, 256, n_dst, dtype=np.uint8), rng.integers(0, 256, n_src, dtype=np.uint8)
    f = lambda n: (rng.standard_normal(n) * 0.2 + 0.5).clip(0, 1).astype(np.float32)
    return f(n_dst), f(n_src)


# ---- 1. every position against the oracle ----------------------------------------------------------------------------
SIZES = [(1, 1), (40, 40), (1500, 100), (20000, 1537), (30000, 9000), (12000, 4097), (140500, 140000)]


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_every_position_against_the_oracle(oracle, dtype, method):
    rng = np.random.default_rng(5)
    dst_row, src_row = _rows(rng, dtype, 200000, 160000)
    src_row[100:100 + 9000] = dst_row[3000:3000 + 9000]             # a real match inside one window
    dst, src = _streams(dst_row, src_row)
    offs, lens, wst, npos = [], [], [], []
    for L, M in SIZES:
        to = int(rng.integers(0, src_row.shape[0] - M + 1)) if M < 9000 else 100 if M == 9000 else 7
        ws = int(rng.integers(0, dst_row.shape[0] - L + 1)) if L != 30000 else 1000
        offs.append(to); lens.append(M); wst.append(ws); npos.append(L - M + 1)
    curves = _curves(dst, src, offs, lens, wst, npos, method)
    for k, (o, m, w, p) in enumerate(zip(offs, lens, wst, npos)):
        ref = oracle.match_template_direct(dst_row[w:w + p + m - 1], src_row[o:o + m], method=method)[0]
        assert curves[k].shape == ref.shape
        if dtype == np.uint8:
            bad = np.flatnonzero(_bits(curves[k]) != _bits(ref))
            assert bad.size == 0, (k, m, p, bad[:5], curves[k][bad[:5]], ref[bad[:5]])
        else:
            tol = 1e-4 * np.abs(ref) + 2.5e-7
            assert np.all(np.abs(curves[k] - ref) <= tol), (k, m, p)


# ---- 2. every position, bitwise, against the NumPy restatement (float32) ------------------------------------------------
@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
def test_float32_every_position_bitwise_against_the_canonical_chain(method):
    rng = np.random.default_rng(9)
    dst_row, src_row = _rows(rng, np.float32, 12000, 6000)
    dst, src = _streams(dst_row, src_row)
    s1, s2 = _prefix(dst, src)
    cases = [(0, 1, 0, 1), (17, 40, 5, 300), (100, 513, 2000, 1100), (1000, 1537, 9000, 1464), (3, 2100, 0, 9901)]
    offs, lens, wst, npos = zip(*cases)
    curves = _curves(dst, src, list(offs), list(lens), list(wst), list(npos), method)
    for k, (o, m, w, p) in enumerate(cases):
        corr = _canonical_corr(src_row[o:o + m].astype(np.float64), dst_row[w:].astype(np.float64), np.arange(p))
        want = _finish(corr, s1, s2, o, w, np.arange(p), m, method)
        bad = np.flatnonzero(_bits(curves[k]) != _bits(want))
        assert bad.size == 0, (k, bad[:5], curves[k][bad[:5]], want[bad[:5]])


# ---- 3. consistency with the search path ----------------------------------------------------------------------------
def _check_against_search(dst, src, offs, lens, wst, npos, method):
    from sushi_amd.device import SearchBatch
    curves = _curves(dst, src, offs, lens, wst, npos, method)
    b = SearchBatch(dst, src, offs, lens, wst, npos, path="fft", method=method)
    b.run()
    idx, score = b.results()
    for k in range(len(offs)):
        assert int(idx[k]) == _first_extremum(curves[k], method), (k, idx[k], _first_extremum(curves[k], method))
        assert _bits(score[k]) == _bits(curves[k][int(idx[k])]), (k, score[k], curves[k][int(idx[k])])
    return curves


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_ragged_batch_matches_the_search_path(dtype):
    rng = np.random.default_rng(11)
    n_dst, n_src = 120000, 30000
    dst_row, src_row = _rows(rng, dtype, n_dst, n_src)
    for k in range(4):
        a, m = 3000 * k + 17, 400 + 250 * k
        src_row[a:a + m] = dst_row[50000 + 1111 * k: 50000 + 1111 * k + m]
    offs, lens, wst, npos = [], [], [], []
    for k in range(24):
        m = int(rng.choice([1, 2, 31, 32, 33, 100, 513, 1024, 2500, 6000]))
        p = int(rng.choice([1, 2, 1023, 1024, 1025, 4097, 20000]))
        offs.append(int(rng.integers(0, n_src - m))); lens.append(m)
        wst.append(int(rng.integers(0, n_dst - (p + m - 1)))); npos.append(p)
    # windows touching both stream ends
    offs += [5, 40]; lens += [700, 3000]; wst += [0, n_dst - (30000 + 3000 - 1)]; npos += [30000, 30000]
    for k in range(4):
        offs.append(3000 * k + 17); lens.append(400 + 250 * k); wst.append(30000); npos.append(60000)
    dst, src = _streams(dst_row, src_row)
    for method in ("sqdiff_normed", "ccoeff_normed"):
        _check_against_search(dst, src, offs, lens, wst, npos, method)


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_tie_saturated_material_matches_the_search_path(sample_type):
    """Silence, a held tone with an exact period and a repeated jingle: deep ties, where the first extremum matters."""
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    rate, seconds, off = 12000, 200.0, 1.75
    dst_pcm, spans = synth.make_hard_dst_pcm(seconds, rate, seed=71, period_s=40.0)
    src_pcm = synth.make_src_pcm(dst_pcm, int(off * rate), seed=72)
    dws = WavStream.from_samples(dst_pcm, rate, sample_rate=rate, sample_type=sample_type)
    sws = WavStream.from_samples(src_pcm, rate, sample_rate=rate, sample_type=sample_type)
    events = synth.make_events(16, seconds, 30 + off, seed=73, min_len=1.0, max_len=2.0)
    events, hard = synth.plant_hard_events(events, spans, off, 0.5, seed=74)
    assert hard.sum() >= 6
    pats, centres, wins = synth.explicit_descriptors(sws, dws, events, off, 30.0, seed=75)
    offs = [sws._get_sample_for_time(s) for s, _ in events]
    lens = [p.shape[1] for p in pats]
    wst, npos = [], []
    for m, c, w in zip(lens, centres, wins):
        _, lo, p = dws._window(m, c, w)
        wst.append(lo); npos.append(p)
    # plus windows at both ends of the stream (the padding: flat windows for TM_CCOEFF_NORMED)
    n = dws.data.shape[1]
    offs += [offs[0], offs[1]]; lens += [lens[0], lens[1]]; wst += [0, n - (20000 + lens[1] - 1)]; npos += [20000, 20000]
    for method in ("sqdiff_normed", "ccoeff_normed"):
        _check_against_search(dws.device_stream(), sws.device_stream(), offs, lens, wst, npos, method)


# ---- 4. full size --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_full_size_windows_first_extremum_of_every_position(sample_type):
    """Two 2-h streams, 16 searches of P = 2,880,001 (+-120 s) and M = 36,000 (3 s): the FFT path's answer is the first
    minimum of the exact curve over every position; 2,000 sampled positions per search against the NumPy restatement."""
    from sushi_amd import synth
    from sushi_amd.device import SearchBatch
    from sushi_amd.wav import WavStream
    rate, seconds, off = 12000, 7200.0, 37.25
    dst_pcm = synth.make_dst_pcm(seconds, rate, seed=101)
    src_pcm = synth.make_src_pcm(dst_pcm, int(off * rate), seed=102)
    dws = WavStream.from_samples(dst_pcm, rate, sample_rate=rate, sample_type=sample_type)
    sws = WavStream.from_samples(src_pcm, rate, sample_rate=rate, sample_type=sample_type)
    rng = np.random.default_rng(103)
    M, P = 36000, 2880001
    n_dst = dws.data.shape[1]
    offs = [int(x) for x in rng.integers(200000, sws.data.shape[1] - M - 200000, 16)]
    wst = [int(min(max(o + int(off * rate) - P // 2 + int(rng.integers(-600000, 600000)), 0), n_dst - (P + M - 1))) for o in offs]
    lens, npos = [M] * 16, [P] * 16
    dst, src = dws.device_stream(), sws.device_stream()
    curves = _curves(dst, src, offs, lens, wst, npos)
    b = SearchBatch(dst, src, offs, lens, wst, npos, path="fft", exclusion="auto")
    b.run()
    idx, score = b.results()
    s1, s2 = _prefix(dst, src)
    d_row, s_row = dws.data[0].astype(np.float64), sws.data[0].astype(np.float64)
    for k in range(16):
        c = curves[k]
        assert c.shape == (P,)
        first = int(np.argmin(c))
        assert int(idx[k]) == first, (k, int(idx[k]), first, score[k], c[first])
        assert _bits(score[k]) == _bits(c[first])
        pos = np.unique(np.concatenate(([0, P - 1, first], rng.integers(0, P, 1997))))
        corr = _canonical_corr(s_row[offs[k]:offs[k] + M], d_row[wst[k]:], pos)
        want = _finish(corr, s1, s2, offs[k], wst[k], pos, M, "sqdiff_normed")
        bad = np.flatnonzero(_bits(c[pos]) != _bits(want))
        assert bad.size == 0, (k, pos[bad[:5]], c[pos[bad[:5]]], want[bad[:5]])


# ---- 5. drop-in ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_match_template_is_find_substreams_result_row(tmp_path, sample_type):
    import torch
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    rate, seconds, off = 12000, 120.0, 2.5
    dst_pcm = synth.make_dst_pcm(seconds, rate, seed=21)
    src_pcm = synth.make_src_pcm(dst_pcm, int(off * rate), seed=22)
    synth.write_wav(str(tmp_path / "dst.wav"), dst_pcm, rate)
    synth.write_wav(str(tmp_path / "src.wav"), src_pcm, rate)
    dws = WavStream(str(tmp_path / "dst.wav"), sample_type=sample_type)
    sws = WavStream(str(tmp_path / "src.wav"), sample_type=sample_type)
    cases = [(30.0, 33.0, 30.0 + off, 10.0),           # inside
             (1.0, 3.5, 1.0 + off, 10.0),              # clipped at -PADDING_SECONDS
             (110.0, 113.0, 110.0 + off, 10.0),        # clipped at the end
             (60.0, 61.5, 60.0 + off, 1.0)]
    pats, cs, ws = [], [], []
    for s, e, c, w in cases:
        p = sws.get_substream(s, e)
        r = dws.match_template(p, c, w)
        st, lo, P = dws._window(p.shape[1], c, w)
        assert r.dtype == np.float32 and r.shape == (1, P)
        diff, t = dws.find_substream(p, c, w)
        k = int(r.argmin(axis=1)[0])
        assert _bits(r[0][k]) == _bits(diff)
        assert st + k / float(dws.sample_rate) == t
        pats.append(p); cs.append(c); ws.append(w)
    many = dws.match_templates(pats, cs, ws)
    for k, (s, e, c, w) in enumerate(cases):
        assert np.array_equal(_bits(many[k]), _bits(dws.match_template(pats[k], c, w)))
    on_dev = dws.match_templates(pats, cs, ws, as_tensor=True)
    assert all(t.is_cuda and t.dtype == torch.float32 and t.shape == m.shape for t, m in zip(on_dev, many))
    assert all(np.array_equal(_bits(t.cpu().numpy()), _bits(m)) for t, m in zip(on_dev, many))
    # TM_CCOEFF_NORMED: the value itself, its first maximum is find_substreams' answer
    r = dws.match_template(pats[0], cs[0], ws[0], method="ccoeff_normed")
    diff, t = dws.find_substreams([pats[0]], [cs[0]], [ws[0]], method="ccoeff_normed")
    k = int(r.argmax(axis=1)[0])
    assert _bits(r[0][k]) == _bits(diff[0]) and r.max() <= 1.0


# ---- 6. asynchronous, stateless, argument checks with real pointers --------------------------------------------------
def test_two_streams_two_workspaces_and_bad_arguments():
    import torch
    from sushi_amd import _native
    from sushi_amd.common import SushiError
    from sushi_amd.curves import match_curves
    rng = np.random.default_rng(31)
    dst_row, src_row = _rows(rng, np.uint8, 300000, 50000)
    dst, src = _streams(dst_row, src_row)
    offs, lens, wst, npos = [10, 2000, 40000], [3000, 36000, 1], [0, 5000, 299999], [200000, 240001, 1]
    ref, ref_o = match_curves(dst, src, offs, lens, wst, npos)
    ref = ref.cpu().numpy()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a, _ = match_curves(dst, src, offs, lens, wst, npos)
    with torch.cuda.stream(s2):
        b, _ = match_curves(dst, src, offs, lens, wst, npos)
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(ref)) and np.array_equal(_bits(b.cpu().numpy()), _bits(ref))
    assert list(ref_o) == [0, 200000, 440001, 440002]
    with pytest.raises(SushiError):
        match_curves(dst, src, [0], [100], [dst_row.shape[0] - 50], [1])
    with pytest.raises(SushiError):
        match_curves(dst, src, [src_row.shape[0] - 10], [100], [0], [1])
    # the C ABI with real device pointers
    L = _native.lib()
    req = np.zeros(2, _native.REQUEST_DTYPE)
    req["tmpl_off"], req["tmpl_len"], req["win_start"], req["n_pos"] = [0, 7], [100, 50], [0, 9], [1000, 2000]
    need = L.sushi_hip_curve_bytes(req.ctypes.data, 2)
    mem = torch.zeros(need + 512, dtype=torch.uint8, device=dst.device)
    out = torch.full((3000 + 16,), 7.0, dtype=torch.float32, device=dst.device)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda m, nb, o: L.sushi_hip_match_curves(dst.handle, src.handle, req.ctypes.data, 2, 0, m, nb, o, st)
    assert call(mem.data_ptr(), need - 1, out.data_ptr()) == -4
    assert call(mem.data_ptr() + 16, need, out.data_ptr()) == -2
    assert call(mem.data_ptr(), need, out.data_ptr() + 2) == -2
    torch.cuda.synchronize()
    assert bool((mem == 0).all()) and bool((out == 7.0).all())            # nothing was written
    assert call(mem.data_ptr(), need, out.data_ptr() + 4) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[0] == 7.0 and np.all(got[3001:] == 7.0) and np.all(got[1:3001] <= 1.0)
