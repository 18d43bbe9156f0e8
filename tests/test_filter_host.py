"""Filtering without a GPU: the NumPy restatement of sushi_hip_filter's arithmetic (sushi_amd/filter.py), the kernel's own
arithmetic header compiled for the CPU (tests/host_filter_check.cpp, a stand-alone program under AddressSanitizer + UBSan), the
entry point's argument checks, the taps' properties, WavStream.filtered's host path, and what the filter is for: the hum scenario
of tests/filter_cases.py searched with the CPU oracle."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import filter_cases as FC
import host_checks
from sushi_amd import _native, filter as F
from sushi_amd.common import SushiError

HERE = os.path.dirname(os.path.abspath(__file__))


# ---------------------------------------------------------------------------------------------- filter_host by hand
def test_hand_computed_cases():
    for x, in_start, taps, want in FC.hand_cases():
        got = F.filter_host(x, in_start, taps, len(want))
        assert got.dtype == x.dtype and got.tolist() == want, (x, taps, got)
    assert F.preemphasis_taps().tolist() == [-0.97, 1.0, 0.0] and F.preemphasis_taps().dtype == np.float64


def _pairwise(v):
    return v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:])


def test_sum_order_is_pinned():
    x, in_start, h = FC.order_case()
    assert [float(v) for v in x] == FC.ORDER_SAMPLES                       # the samples hold them exactly
    d = [float(v) - 0.5 for v in x]
    h = [float(v) for v in h]
    p = [a * b for a, b in zip(h, d)]
    seq = rev = fma = 0.0
    for k in range(5):
        seq = seq + p[k]
        rev = rev + p[4 - k]
        fma = float(Fraction(h[k]) * Fraction(d[k]) + Fraction(fma))       # one rounding for product and sum
    got = [float(np.float32(v + 0.5)) for v in (seq, rev, _pairwise(p), fma)]
    assert got == [FC.ORDER_SEQUENTIAL, FC.ORDER_REVERSED, FC.ORDER_PAIRWISE, FC.ORDER_FMA] and len(set(got)) == 4
    assert F.filter_host(x, in_start, h, 1).tolist() == [FC.ORDER_SEQUENTIAL]


BAD = [  # (in_start, n_taps, out_len) on a row of 100 samples
    (-1, 3, 1), (100, 3, 1), (0, 2, 1), (0, 0, 1), (0, 2049, 1), (0, 4, 1), (0, 3, 0), (0, 3, -1), (0, 3, 1 << 40)]


def test_filter_host_refuses_bad_arguments():
    x = np.zeros(100, np.uint8)
    for in_start, n_taps, out_len in BAD:
        with pytest.raises(SushiError):
            F.filter_host(x, in_start, np.ones(n_taps), out_len)
    for taps in ([1.0, np.nan, 0.0], [np.inf], [[1.0, 0.0, 0.0]], []):
        with pytest.raises(SushiError):
            F.filter_host(x, 0, taps, 1)
    with pytest.raises(SushiError):
        F.filter_host(np.zeros(10, np.int16), 0, [1.0], 1)
    with pytest.raises(SushiError):
        F.filter_host(np.zeros((1, 10), np.uint8), 0, [1.0], 1)
    assert F.filter_host(x, 99, np.ones(2047) / 2047, 3).tolist() == [0, 0, 0] and F.filter_host(x, 0, [1.0], 1).shape == (1,)


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic on the CPU
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("filter")), "host_filter_check")
    subprocess.check_call(["g++"] + host_checks.KERNEL_ARITHMETIC + [os.path.join(HERE, "host_filter_check.cpp"), "-o", exe])
    return exe


def _run_check(exe, tmp_path, x, cases):
    """cases: (in_start, taps, out_len) or, for a probe of stage_filter alone, (in_start, n_taps, out_len, nulls, dtype, n_in).
    Returns (outputs, stage records)."""
    fin, ftaps, fcase, fout, fstage = (os.path.join(str(tmp_path), n) for n in ("in.bin", "taps.bin", "case.bin", "out.bin", "stage.bin"))
    x.tofile(fin)
    all_taps, recs = [np.zeros(max([1] + [c[1] for c in cases if len(c) == 6]))], []      # (what a probe's n_taps points at)
    for c in cases:
        if len(c) == 3:
            h = np.asarray(c[1], np.float64)
            recs.append((c[0], sum(t.shape[0] for t in all_taps), h.shape[0], c[2], 0, -1, 0))
            all_taps.append(h)
        else:
            recs.append((c[0], 0, c[1], c[2], c[3], c[4], c[5]))
    np.concatenate(all_taps).tofile(ftaps)
    np.array(recs, dtype=np.int64).reshape(-1, 7).tofile(fcase)
    r = subprocess.run([exe, "u8" if x.dtype == np.uint8 else "f32", fin, ftaps, fcase, fout, fstage], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(fout, dtype=x.dtype), np.fromfile(fstage, dtype=np.int64).reshape(-1, 4)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("n_taps", FC.TAP_COUNTS)
def test_kernel_arithmetic_equals_filter_host_bitwise(host_check, tmp_path, dtype, n_taps):
    h = FC.taps(n_taps)
    tile, most = FC.launch_shape(n_taps)
    assert (tile, most) == {1: (2048, 1280), 3: (2048, 1280), 63: (2048, 1280), 255: (2048, 1280), 2047: (1024, 768)}[n_taps]
    for n_in in FC.ROWS:
        x = FC.samples(n_in, dtype, seed=n_in)
        cases = [(in_start, h, out_len) for in_start, out_len in FC.grid(n_in)]
        got, stages = _run_check(host_check, tmp_path, x, cases)
        want = np.concatenate([F.filter_host(x, *c) for c in cases])
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), n_in
        for (_in_start, _h, out_len), (rc, t, n_tiles, grid) in zip(cases, stages):
            assert rc == 0 and t == tile and n_tiles == -(-out_len // tile) and grid == min(n_tiles, most)
        if dtype == np.uint8 and n_in == 70001 and n_taps <= 3:  # a gain of up to 2: both ends of the range are met
            assert want.min() == 0 and want.max() == 255


def test_hand_cases_and_the_pinned_order_by_the_header(host_check, tmp_path):
    for x, in_start, taps, want in FC.hand_cases():
        got, _ = _run_check(host_check, tmp_path, x, [(in_start, taps, len(want))])
        assert got.tolist() == want, (x, taps)
    x, in_start, h = FC.order_case()
    got, _ = _run_check(host_check, tmp_path, x, [(in_start, h, 1)])
    assert got.tolist() == [FC.ORDER_SEQUENTIAL]
    # what the Python side refuses, the arithmetic defines: a NaN tap gives 0 on uint8, NaN on float32
    got, _ = _run_check(host_check, tmp_path, np.array([0, 128, 255], np.uint8), [(0, [np.nan], 3), (0, [0.0, np.nan, 0.0], 3)])
    assert got.tolist() == [0] * 6
    got, _ = _run_check(host_check, tmp_path, np.array([0.25, 0.5], np.float32), [(0, [np.nan], 2)])
    assert np.isnan(got).all() and got.shape == (2,)


def test_stage_filter_refuses_what_the_entry_point_refuses(host_check, tmp_path):
    x = np.zeros(100, np.uint8)
    bad = [(s, t, m, 0, -1, 0) for s, t, m in BAD] + [
        (0, 3, 1, 1, -1, 0), (0, 3, 1, 2, -1, 0), (0, 3, 1, 4, -1, 0),            # a null pointer: the row, the taps, the output
        (0, 3, 1, 0, 2, 0), (0, 3, 1, 0, 7, 0),                                      # an unknown dtype
        (0, 3, 1, 0, -1, -5), (0, 3, 1, 0, -1, 1 << 62), (0, 2047, 1, 0, -1, 0)]   # n_in; (the last: fine)
    fine = [(99, 2047, (1 << 40) - 1, 0, 1, (1 << 62) - 1), (0, 1025, 1 << 30, 0, 0, 0), (0, 1027, 1 << 30, 0, 0, 0)]
    _got, stages = _run_check(host_check, tmp_path, x, bad + fine)
    assert stages[:-4, 0].tolist() == [-1] * (len(bad) - 1)
    assert stages[-4].tolist() == [0, 1024, 1, 1] and stages[-3].tolist() == [0, 1024, 1 << 30, 768]
    # the widest wide tile (35,848 bytes of LDS: four workgroups a CU) and the narrowest narrow one (28,720: five)
    assert stages[-2].tolist() == [0, 2048, 1 << 19, 1024] and stages[-1].tolist() == [0, 1024, 1 << 20, 1280]


# ---------------------------------------------------------------------------------------------- the entry point's checks
def test_filter_entry_point_validates_before_any_hip_call():
    """No pointer is dereferenced and no launch is made: every probe either fails a check (EINVAL) or, its arguments in range,
    stops at the alignment check behind them (EALIGN: float32 samples at an odd address)."""
    L = _native.lib()
    C = ctypes
    P, Q, H, ODD = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20), C.c_void_p((2 << 20) + 2)   # never dereferenced
    BIG = 1 << 50

    def call(n_in=1000, in_start=0, n_taps=255, out_len=100, dtype=_native.F32, src=P, taps=H, out=ODD):
        return L.sushi_hip_filter(src, dtype, n_in, in_start, taps, n_taps, out, out_len, None)

    assert call() == -2 and call(src=C.c_void_p((1 << 20) + 1), out=Q) == -2
    assert call(dtype=_native.U8, taps=C.c_void_p((3 << 20) + 4)) == -2         # the taps: 8 bytes
    for kw in ({"src": None}, {"out": None}, {"taps": None}, {"dtype": 2}, {"dtype": -1}, {"n_in": 0}, {"n_in": -5}, {"out_len": 0},
               {"out_len": -1}, {"out_len": 1 << 40}, {"in_start": -1}, {"in_start": 1000}, {"n_taps": 0}, {"n_taps": -3},
               {"n_taps": 2}, {"n_taps": 256}, {"n_taps": 2048}, {"n_taps": 2049}, {"n_in": 1 << 62}):
        assert call(**kw) == -1, kw
    # ... and the inclusive ends of every range pass the checks
    for kw in ({"n_in": 1}, {"in_start": 999}, {"n_taps": 1}, {"n_taps": 2047}, {"n_taps": 1025}, {"n_taps": 1027}, {"out_len": 1},
               {"out_len": (1 << 40) - 1}, {"n_in": BIG, "in_start": BIG - 1}):
        assert call(**kw) == -2, kw
    assert call(dtype=_native.U8, n_taps=4) == -1 and call(dtype=_native.U8, out_len=0) == -1
    assert "sushi_hip_filter" in _native.declared_symbols() and "sushi_hip_filter_bytes" not in _native.declared_symbols()


# ---------------------------------------------------------------------------------------------- the taps
def _gain(h, f, rate):
    k = np.arange(h.shape[0], dtype=np.float64)
    return abs(complex(np.sum(h * np.exp(-2j * np.pi * f / rate * k))))


def test_band_taps_properties():
    rate = 12000
    lp, hp = F.band_taps(rate, high=3000), F.band_taps(rate, low=150)
    bp, bs = F.band_taps(rate, 300, 3000), F.band_taps(rate, 300, 3000, stop=True)
    for h in (lp, hp, bp, bs, F.band_taps(rate, low=150, n_taps=3), F.band_taps(rate, high=100, n_taps=2047)):
        assert h.dtype == np.float64 and h.shape[0] & 1 and np.isfinite(h).all()
        assert (h == h[::-1]).all()                                       # symmetric: linear phase, no shift of its own
    assert lp.shape == hp.shape == bp.shape == bs.shape == (255,)
    assert abs(lp.sum() - 1.0) < 1e-12 and abs(bs.sum() - 1.0) < 1e-12      # DC gain 1
    assert abs(hp.sum()) < 1e-12 and abs(bp.sum()) < 1e-12                  # DC gain 0
    delta = np.zeros(255)
    delta[127] = 1.0
    assert (F.band_taps(rate, low=150, stop=True) == delta - hp).all() and (bs == delta - bp).all()
    # mains hum through the default high-pass: at least 40 dB down, the programme's band untouched
    hum = 20.0 * np.log10(_gain(hp, 50.0, rate))
    print("50 Hz through low=150, 255 taps at 12 kHz: %.1f dB; 60 Hz: %.1f dB; 400 Hz: %.4f dB"
          % (hum, 20.0 * np.log10(_gain(hp, 60.0, rate)), 20.0 * np.log10(_gain(hp, 400.0, rate))))
    assert hum <= -40.0
    assert abs(20.0 * np.log10(_gain(hp, 400.0, rate))) < 0.1 and abs(20.0 * np.log10(_gain(hp, 5000.0, rate))) < 0.1
    # band-pass and band-stop at the band's middle and outside it
    assert abs(_gain(bp, 1500.0, rate) - 1.0) < 1e-3 and _gain(bp, 5500.0, rate) < 1e-3
    assert _gain(bs, 1500.0, rate) < 1e-3 and abs(_gain(bs, 5500.0, rate) - 1.0) < 1e-3
    for bad in ({"low": 150, "n_taps": 254}, {"low": 150, "n_taps": 1}, {"low": 150, "n_taps": 2049}, {}, {"stop": True},
                {"low": 0}, {"low": -5}, {"high": 6000}, {"high": 7000}, {"low": 3000, "high": 300}, {"low": 300, "high": 300},
                {"low": 300, "high": 6000}):
        with pytest.raises(SushiError):
            F.band_taps(rate, **bad)


# ---------------------------------------------------------------------------------------------- WavStream.filtered, host path
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_filtered_on_the_host(monkeypatch, sample_type):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream, _locate
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    rate = 12000
    src = WavStream.from_samples(synth.make_dst_pcm(10, rate, seed=5), rate, sample_type=sample_type)
    pad, count = src.padding_size, src.sample_count
    for kw, taps in (({"low": 150}, F.band_taps(rate, low=150)),
                     ({"low": 300, "high": 3000, "stop": True, "n_taps": 63}, F.band_taps(rate, 300, 3000, 63, True)),
                     ({"taps": F.preemphasis_taps()}, F.preemphasis_taps()),
                     ({"low": 150, "taps": [0.25, 0.5, 0.25]}, [0.25, 0.5, 0.25])):          # taps= overrides the design
        f = src.filtered(**kw)
        assert (f.sample_rate, f.padding_size, f.sample_count) == (rate, pad, count)
        assert f.data.shape == src.data.shape and f.data.dtype == src.data.dtype and f._dev_row is None
        body = F.filter_host(src.data[0], pad, taps, count)
        assert f.data[0, pad:pad + count].tobytes() == body.tobytes()
        assert (f.data[0, :pad] == body[0]).all() and (f.data[0, pad + count:] == body[-1]).all()
        assert f.duration_seconds == src.duration_seconds
    # the identity holds the same samples (the pads too: they were filled from the body's ends)
    same = src.filtered(taps=[1.0])
    assert same is not src and same.data.tobytes() == src.data.tobytes()
    # the first outputs read the left pad, not a clamp at the body's start
    h = np.zeros(255)
    h[0] = 1.0                                                          # output i reads the sample 127 places in front of it
    assert src.filtered(taps=h).data[0, pad:pad + count].tobytes() == src.data[0, pad - 127:pad + count - 127].tobytes()
    # a pattern cut from the result is an ordinary view of a live stream
    f = src.filtered(low=150)
    owner, off, length = _locate(f.get_substream(2.5, 4.5))
    assert owner is f and off == f.padding_size + int(rate * 2.5) and length == 2 * rate
    for bad in ({}, {"low": 150, "n_taps": 254}, {"high": rate / 2}, {"taps": [1.0, 2.0]}, {"taps": [np.nan]}, {"taps": np.ones(2049)}):
        with pytest.raises(SushiError):
            src.filtered(**bad)
    # it composes: a band contour, and a filtered stream on another clock
    assert f.envelope(8, 4).sample_rate == rate // 8 and f.retimed("25/24").sample_count == ((count - 1) * 25) // 24 + 1


# ---------------------------------------------------------------------------------------------- what the filter is for
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_high_pass_gives_back_what_the_hum_hides(oracle, monkeypatch, sample_type):
    """Two captures with a mains hum of their own at 2 x the programme's rms (tests/filter_cases.py): the plain search places at
    most 16 of 24 events at the planted shift (measured with this path: 8 for both sample types; 3 at 4 x), and every one of the
    24 after filtered(low=150) on both streams."""
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    search = lambda row, pat: oracle.argmin_first(oracle.match_template_fft(row, pat, method=FC.SQ)[0])
    dst, src = FC.stream("dst", sample_type), FC.stream("src", sample_type)
    evs = FC.events()
    raw = FC.found_shifts(dst, *FC.requests(src, evs), search)
    f_dst, f_src = dst.filtered(low=FC.LOW, n_taps=FC.N_TAPS), src.filtered(low=FC.LOW, n_taps=FC.N_TAPS)
    assert f_dst._dev_row is None                                       # filter_host
    got = FC.found_shifts(f_dst, *FC.requests(f_src, evs), search)
    n_raw, n_filtered = int((raw == FC.OFFSET).sum()), int((got == FC.OFFSET).sum())
    print(sample_type, "unfiltered", n_raw, "filtered", n_filtered)
    assert n_filtered == 24, got
    assert n_raw <= 16, raw
