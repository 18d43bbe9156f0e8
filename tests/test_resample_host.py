"""Filtered decimation without a GPU: the table, the NumPy restatement of sushi_hip_load_resample_fir's arithmetic
(sushi_amd/resample.py), the kernel's own arithmetic header compiled for the CPU (tests/host_resample_check.cpp, under
AddressSanitizer + UBSan), the entry point's argument checks, the host pipeline with resample='fir', and the case the feature is
for: one programme at 48 kHz and at 44.1 kHz, matched after loading both to 12 kHz."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import resample_cases as cases
from host_checks import build_check
from sushi_amd import _native, resample
from sushi_amd.common import SushiError, py2_round

TRIPLES = {(48000, 12000): (4, 1, 72), (44100, 12000): (147, 40, 66), (44100, 8000): (441, 80, 98), (22050, 12000): (147, 80, 33),
           (96000, 12000): (8, 1, 143), (32000, 12000): (8, 3, 48), (11025, 12000): (147, 160, 18), (8000, 12000): (2, 3, 18)}


def _longest(n_raw, num, den):
    """Most body samples an input allows: the last one's centre (n_body - 1) * num // den stays at or below n_raw - 1."""
    return (n_raw * den - 1) // num + 1


# ---------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("rates", sorted(TRIPLES))
def test_table_shape_sums_and_mirror(rates):
    num, den, W, H = resample.fir_table(*rates)
    assert (num, den, W) == TRIPLES[rates] == resample.ratio(*rates) + (W,)
    assert H.shape == (den, 2 * W) and H.dtype == np.float64 and H.flags.c_contiguous and not H.flags.writeable
    assert np.abs(H.sum(axis=1) - 1.0).max() <= 1e-15
    # an output r / den behind a frame is the mirror image of one (den - r) / den behind it: H[den - r][2W - 1 - c] = H[r][c]
    for r in range(1, den):
        assert np.abs(H[den - r][::-1] - H[r]).max() <= 1e-15, r
    # the formula itself, one entry at a time on Python floats (before the division by the row's sum)
    import math
    fc = 0.9 * 0.5 * min(1.0, den / num)
    assert W == math.ceil(16 / (2 * fc))
    for r, c in ((0, 0), (0, W - 1), (den - 1, 2 * W - 1), (den // 2, W // 3)):
        d = (c - W + 1) - r / den
        row = [float(np.sinc(2 * fc * ((k - W + 1) - r / den))) * (0.5 + 0.5 * math.cos(math.pi * ((k - W + 1) - r / den) / W))
               for k in range(2 * W)]
        want = float(np.sinc(2 * fc * d)) * (0.5 + 0.5 * math.cos(math.pi * d / W)) / math.fsum(row)
        assert abs(H[r, c] - want) <= 1e-15


def test_table_over_the_limit_is_refused():
    with pytest.raises(SushiError):
        resample.fir_table(44100, 12001)              # den = 12001 rows
    with pytest.raises(SushiError):
        resample.fir_table(192000 * 20, 1000)         # 2W = 136534 columns
    with pytest.raises(SushiError):
        resample.fir_table((1 << 20) + 1, 1 << 20)
    with pytest.raises(SushiError):
        resample.ratio(0, 12000)
    num, den, W, H = resample.fir_table(200 * 12000, 12000)     # a wide table inside the limit
    assert (num, den, W) == (200, 1, 3556) and den * 2 * W <= 65536


# ---------------------------------------------------------------------------------------------- resample_host
@pytest.mark.parametrize("rates", [(48000, 12000), (44100, 12000), (8000, 12000)])
def test_restatement_equals_python_floats_at_scattered_outputs(rates):
    """The same operations on Python's integers and floats (float64, one rounding per product and per sum), including outputs
    whose taps clamp at the input's first and at its last sample."""
    num, den, W, H = resample.fir_table(*rates)
    n_raw = 5003
    x = cases.int16_noise(n_raw, seed=4)
    n_body = _longest(n_raw, num, den)
    assert (n_body - 1) * num // den == n_raw - 1 or ((n_body - 1) * num // den < n_raw and n_body * num // den >= n_raw)
    out = resample.resample_host(x, rates[0], rates[1], n_body)
    assert out.dtype == np.float32 and out.shape == (n_body,)
    picks = sorted(set(list(range(0, 12)) + list(range(n_body - 12, n_body)) + list(range(0, n_body, 97))))
    clamped_low = clamped_high = 0
    for i in picks:
        t = i * num
        j, r = t // den, t % den
        acc = 0.0
        for c in range(2 * W):
            k = j - W + 1 + c
            clamped_low += k < 0
            clamped_high += k > n_raw - 1
            acc = acc + float(H[r, c]) * float(x[min(max(k, 0), n_raw - 1)])
        assert out[i] == np.float32(acc), (i, out[i], acc)
    assert clamped_low and clamped_high
    # a slice of the body is the body's slice
    part = resample.resample_host(x, rates[0], rates[1], n_body, first=n_body - 300, count=200)
    assert part.tobytes() == out[n_body - 300:n_body - 100].tobytes()
    assert resample.resample_host(x, rates[0], rates[1], n_body, first=3, count=50, stride=7).tobytes() == out[3:353:7].tobytes()
    assert resample.resample_host(x, rates[0], rates[1], n_body, first=3, stride=7).tobytes() == out[3::7].tobytes()
    with pytest.raises(SushiError):
        resample.resample_host(x, rates[0], rates[1], n_body + 1 + den // num)        # a last centre behind the input
    with pytest.raises(SushiError):
        resample.resample_host(x, rates[0], rates[1], n_body, first=5, count=n_body)
    with pytest.raises(SushiError):
        resample.resample_host(x.astype(np.float64), rates[0], rates[1], n_body)


@pytest.mark.parametrize("rates", [(48000, 12000), (44100, 12000), (11025, 12000)])
def test_constant_input_comes_out_bit_equal(rates):
    """Every row sums to 1 and the value is representable, so a constant passes unchanged -- at the clamped ends too.  Zeros: the
    sum starts at +0.0 and every product is a zero, so +0.0 comes out as +0.0 bit for bit, and an input of -0.0 comes out as the
    equal value +0.0 (0.0 + -0.0 = +0.0 in the stated arithmetic: the sign of a zero is not the filter's to keep)."""
    num, den, _, _ = resample.fir_table(*rates)
    n_raw = 3000
    n_body = _longest(n_raw, num, den)
    for value in (1234.0, -777.0, 32767.0, -32768.0, 0.5, 0.0):
        x = np.full(n_raw, value, np.float32)
        out = resample.resample_host(x, rates[0], rates[1], n_body)
        assert out.tobytes() == np.full(n_body, value, np.float32).tobytes(), value
    zeros = np.zeros(n_raw, np.float32)
    zeros[::2] = -0.0
    for x in (np.full(n_raw, -0.0, np.float32), zeros):
        out = resample.resample_host(x, rates[0], rates[1], n_body)
        assert (out == x[0]).all() and out.tobytes() == np.zeros(n_body, np.float32).tobytes()


def test_equal_rates_give_the_nearest_paths_bytes(monkeypatch):
    from sushi_amd.wav import WavStream
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    x = cases.int16_noise(int(2.3 * 12000), seed=5)
    assert resample.resample_host(x, 12000, 12000, x.shape[0]).tobytes() == x.tobytes()
    for sample_type in ("uint8", "float32"):
        a = WavStream.from_samples(x, 12000, sample_type=sample_type)
        b = WavStream.from_samples(x, 12000, sample_type=sample_type, resample="fir")
        assert a.data.dtype == b.data.dtype and a.data.tobytes() == b.data.tobytes()
        assert (a.sample_count, a.padding_size) == (b.sample_count, b.padding_size)


def _level(freq, rate):
    """rms of the 12 kHz body of a tone over the input's rms, 2000 samples off each end."""
    x = cases.tone(freq, rate, seconds=1.0)
    y = resample.resample_host(x, rate, 12000, 12000)
    rms = lambda v: float(np.sqrt(np.mean(np.asarray(v, np.float64) ** 2)))
    return rms(y[2000:-2000]) / rms(x)


def test_filter_quality():
    """What lies above 6 kHz is taken out before it can fold, what lies below stays.  Measured with this code: 7 kHz at 48 kHz comes
    out at 3.1e-4 of its level, 6.7 kHz at 48 kHz at 7.4e-4, 9 kHz at 44.1 kHz at 2.8e-5; 3 kHz at 48 kHz passes at 0.99986."""
    got = {"7k@48k": _level(7000, 48000), "6.7k@48k": _level(6700, 48000), "9k@44.1k": _level(9000, 44100), "3k@48k": _level(3000, 48000)}
    print(got)
    assert got["7k@48k"] <= 1e-3
    assert got["9k@44.1k"] <= 1e-3
    assert got["3k@48k"] >= 0.999
    assert got["6.7k@48k"] <= 1e-3


def test_mode_is_checked_everywhere():
    from sushi_amd.wav import WavStream
    x = np.zeros(100, np.float32)
    for bad in ("linear", "FIR", None, 1, b"fir"):
        with pytest.raises(SushiError):
            WavStream.from_samples(x, 48000, resample=bad)
        with pytest.raises(SushiError):
            WavStream.from_channels(np.zeros((100, 2), np.int16), 48000, "side", resample=bad)
        with pytest.raises(SushiError):
            WavStream.load_mixes("/nonexistent.wav", ["mean"], resample=bad)
        with pytest.raises(SushiError):
            WavStream("/nonexistent.wav", resample=bad)


# ---------------------------------------------------------------------------------------------- the entry point's checks
def test_resample_fir_entry_point_validates_before_any_hip_call():
    L = _native.lib()
    C = ctypes
    P, T, Q = 1 << 20, 2 << 20, 3 << 20                 # never dereferenced
    BIG = 1 << 50
    base = dict(raw=P, n_raw=1000, num=4, den=1, table=T, W=72, n_body=250, pad=10, total=270, data=Q)

    def call(**kw):
        a = dict(base, **kw)
        ptr = lambda v: None if v is None else C.c_void_p(v)
        return L.sushi_hip_load_resample_fir(ptr(a["raw"]), a["n_raw"], a["num"], a["den"], ptr(a["table"]), a["W"], a["n_body"],
                                             a["pad"], a["total"], ptr(a["data"]), None)

    # a call that passes every EINVAL check but the alignment ends with EALIGN: what is valid is told apart from what is not
    ok = dict(table=T + 4)
    assert call(**ok) == -2
    assert call(raw=P + 2) == -2 and call(data=Q + 1) == -2 and call(table=T + 4, raw=P + 4, data=Q + 4) == -2
    for kw in ({"raw": None}, {"table": None}, {"data": None}):
        assert call(**dict(ok, **kw)) == -1, kw
    for kw in ({"n_raw": 0}, {"n_raw": -1}, {"n_body": 0}, {"n_body": -7},
               {"num": 0}, {"num": -4}, {"num": (1 << 20) + 1}, {"den": 0}, {"den": -1}, {"den": (1 << 20) + 1},
               {"W": 0}, {"W": -72},
               {"W": 32769},                                                     # 1 x 65538 entries
               {"den": 40, "num": 147, "W": 820},                                # 40 x 1640 = 65600
               {"num": 1 << 20, "den": 1 << 20, "W": 1, "n_body": 1},            # 2^20 x 2
               {"n_body": 251, "total": 9999},                                   # the last centre at 250 * 4 = n_raw
               {"num": 147, "den": 40, "W": 66, "n_body": 274, "total": 9999},   # 273 * 147 // 40 = 1003
               {"pad": -1}, {"total": 269}, {"pad": 11}, {"total": 0}, {"total": -5}, {"pad": 300},
               {"n_body": 1 << 40, "n_raw": BIG, "total": BIG}):
        assert call(**dict(ok, **kw)) == -1, kw
    # ... and the inclusive ends of every range pass the checks (den: 32768 rows of two columns are the table's limit)
    for kw in ({"n_raw": 997}, {"n_body": 1}, {"n_body": 1, "n_raw": 1},
               {"num": 1, "den": 32768, "W": 1}, {"num": 1 << 20, "den": 1, "W": 32768, "n_body": 1},
               {"W": 1}, {"W": 32768}, {"den": 40, "num": 147, "W": 819},
               {"num": 147, "den": 40, "W": 66, "n_body": 273, "total": 293},    # 272 * 147 // 40 = 999
               {"pad": 0, "total": 250}, {"pad": 0, "total": 9999}, {"total": BIG},
               {"n_body": (1 << 40) - 1, "n_raw": BIG, "total": BIG}):
        assert call(**dict(ok, **kw)) == -2, kw


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic on the CPU
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return build_check("host_resample_check", tmp_path_factory.mktemp("resample"))


@pytest.mark.parametrize("rates", [(48000, 12000), (44100, 12000), (44100, 8000), (11025, 12000)])
def test_kernel_arithmetic_equals_resample_host_bitwise(host_check, tmp_path, rates):
    num, den, W, H = resample.fir_table(*rates)
    n_raw = 9001
    x = cases.int16_noise(n_raw, seed=6, leading_zeros=30)
    fin, ftab, fout = (os.path.join(tmp_path, n) for n in ("in.bin", "table.bin", "out.bin"))
    x.tofile(fin)
    H.tofile(ftab)
    longest = _longest(n_raw, num, den)
    assert longest > 1024                                                        # more than one run of the kernel
    for n_body in (longest, 1):
        want = resample.resample_host(x, rates[0], rates[1], n_body)
        r = subprocess.run([host_check, fin, ftab, fout, str(num), str(den), str(W), str(n_body)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(fout, dtype=np.float32)
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
    r = subprocess.run([host_check, fin, ftab, fout, str(num), str(den), str(W), str(longest + 1 + den // num)], capture_output=True)
    assert r.returncode == 2                                                     # (its own check of the last read)


# ---------------------------------------------------------------------------------------------- the host pipeline
def normalise_like_the_pipeline(data, sample_type):
    """wav.py:140-156 on a float32 row whose body is in place: what WavStream._build_host does after the decimation."""
    data = data.copy()
    max_value = float(np.median(data[data >= 0])) * 3
    min_value = float(np.median(data[data <= 0])) * 3
    np.clip(data, min_value, max_value, out=data)
    data -= min_value
    data /= (max_value - min_value)
    if sample_type == "uint8":
        data *= 255.0
        data += 0.5
        data = data.astype("uint8")
    return data


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
@pytest.mark.parametrize("framerate", [48000, 44100])
def test_host_pipeline_with_fir(monkeypatch, framerate, sample_type):
    from sushi_amd.wav import WavStream
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    x = cases.int16_noise(int(3.37 * framerate), seed=7)
    near = WavStream.from_samples(x, framerate, sample_type=sample_type, resample="nearest")
    fir = WavStream.from_samples(x, framerate, sample_type=sample_type, resample="fir")
    assert fir.data.shape == near.data.shape and fir.data.dtype == near.data.dtype
    assert (fir.sample_count, fir.padding_size, fir.sample_rate) == (near.sample_count, near.padding_size, near.sample_rate)
    assert fir.data.tobytes() != near.data.tobytes()
    pad, total = fir.padding_size, fir.data.shape[1]
    n_full, rest = divmod(x.shape[0], framerate)
    assert rest                                                                  # the last chunk is ragged
    n_body = n_full * int(py2_round(framerate * (12000 / float(framerate)))) + int(py2_round(rest * (12000 / float(framerate))))
    row = np.zeros((1, total), np.float32)
    row[0, pad:pad + n_body] = resample.resample_host(x, framerate, 12000, n_body)
    row[0, :pad] = row[0, pad]
    row[0, total - pad:] = row[0, total - pad - 1]
    want = normalise_like_the_pipeline(row, sample_type)
    assert fir.data.tobytes() == want.tobytes()
    assert (fir.data[0, :pad] == fir.data[0, pad]).all() and (fir.data[0, total - pad:] == fir.data[0, total - pad - 1]).all()


# ---------------------------------------------------------------------------------------------- the case the feature is for
def test_one_programme_at_two_rates_matches_only_when_filtered(monkeypatch, oracle):
    """3 s of the 44.1 kHz rendition sought within +-3.5 s in the 48 kHz rendition, both at 12 kHz, float32, host pipeline.
    Measured with this code and the recipe of tests/resample_cases.py (it differs from the first prototype's, which put 0.352 and
    2.1e-7 here): 'nearest' 0.368 at the true offset (best score 50 or more samples away: 0.918), 'fir' 3.3e-6 (0.200).  The bounds
    are the issue's: >= 0.2 keeps a factor 1.8 to the first figure, <= 0.01 a factor 3000 to the second."""
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    got = {}
    for mode in ("nearest", "fir"):
        dst, src = cases.programme_streams(mode)
        row, true = cases.programme_scores(oracle, dst, src)
        far = np.ones(row.shape[0], bool)
        far[true - 49:true + 50] = False
        got[mode] = (int(row.argmin()), true, float(row[true]), float(row[far].min()))
    print(got)
    for mode in ("nearest", "fir"):
        assert got[mode][0] == got[mode][1] == 42000, mode
    assert got["nearest"][2] >= 0.2
    assert got["fir"][2] <= 0.01
