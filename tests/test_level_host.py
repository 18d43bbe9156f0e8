"""Levelling without a GPU: the NumPy restatement of sushi_hip_level's arithmetic (sushi_amd/level.py), the kernels' own arithmetic
header compiled for the CPU (tests/host_level_check.cpp, a stand-alone program under AddressSanitizer + UBSan), the entry point's
argument checks, WavStream.levelled's host path, and what levelling is for: the dub scenario of tests/level_cases.py searched with
the CPU oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import filter_cases as FC
import level_cases as LC
from sushi_amd import _native, level as LV
from sushi_amd.common import SushiError

HERE = os.path.dirname(os.path.abspath(__file__))
# the header IS the kernels' arithmetic and its unit is built without contraction, so the check is too; under the sanitizers
CHECK_FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


# ---------------------------------------------------------------------------------------------- level_host by hand
def test_hand_computed_cases():
    assert (LV.WINDOW, LV.FLOOR, LV.PEAK, LV.MAX_WINDOW) == (129, 1.0 / 128, 8.0, 1023)
    for x, in_start, window, floor, peak, want in LC.hand_cases():
        got = LV.level_host(x, in_start, window, floor, peak, len(want))
        assert got.dtype == x.dtype and got.tolist() == want, (x, window, peak, got)


def _pairwise(v):
    return v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:])


def test_sum_order_is_pinned():
    x, in_start, window, floor, peak = LC.order_case()
    assert [float(v) for v in x] == LC.ORDER_SAMPLES                       # the samples hold them exactly
    d = [float(v) - 0.5 for v in x]
    a = [abs(v) for v in d]
    seq = rev = 0.0
    for t in range(window):
        seq = seq + a[t]
        rev = rev + a[window - 1 - t]
    fw = (floor * 0.5) * float(window)

    def finish(e):
        q = (d[in_start] * float(window)) / ((e + fw) * peak)
        assert -1.0 < q < -0.5                                              # no clamp: 0.5 + 0.5 * q is exact
        return float(np.float32(0.5 + 0.5 * q))

    got = [finish(e) for e in (seq, rev, _pairwise(a))]
    assert got == [LC.ORDER_SEQUENTIAL, LC.ORDER_REVERSED, LC.ORDER_PAIRWISE]
    assert got[0] != got[1] and got[0] != got[2]
    assert LV.level_host(x, in_start, window, floor, peak, 1).tolist() == [LC.ORDER_SEQUENTIAL]


# (in_start, window, floor, peak, out_len) on a row of 100 samples
BAD = [(-1, 3, 0.5, 1.0, 1), (100, 3, 0.5, 1.0, 1), (0, 2, 0.5, 1.0, 1), (0, 0, 0.5, 1.0, 1), (0, -1, 0.5, 1.0, 1),
       (0, 1025, 0.5, 1.0, 1), (0, 1024, 0.5, 1.0, 1), (0, 3, 0.0, 1.0, 1), (0, 3, -0.5, 1.0, 1), (0, 3, np.inf, 1.0, 1),
       (0, 3, np.nan, 1.0, 1), (0, 3, 0.5, 0.0, 1), (0, 3, 0.5, -1.0, 1), (0, 3, 0.5, np.inf, 1), (0, 3, 0.5, np.nan, 1),
       (0, 3, 0.5, 1.0, 0), (0, 3, 0.5, 1.0, -1), (0, 3, 0.5, 1.0, 1 << 40)]


def test_level_host_refuses_bad_arguments():
    x = np.zeros(100, np.uint8)
    for in_start, window, floor, peak, out_len in BAD:
        with pytest.raises(SushiError):
            LV.level_host(x, in_start, window, floor, peak, out_len)
    with pytest.raises(SushiError):
        LV.level_host(np.zeros(10, np.int16), 0, 1, 0.5, 1.0, 1)
    with pytest.raises(SushiError):
        LV.level_host(np.zeros((1, 10), np.uint8), 0, 1, 0.5, 1.0, 1)
    with pytest.raises(SushiError):
        LV.level_host(x, 0, 3, "loud", 1.0, 1)
    # a constant row d = -128: q = -(128 / 129) / 8 whatever the window -> floor(-15.87.. + 128.5)
    assert LV.level_host(x, 99, 1023, 1.0 / 128, 8.0, 3).tolist() == [112, 112, 112] and LV.level_host(x, 0, 1, 5e-324, 1e308, 1).shape == (1,)


# ---------------------------------------------------------------------------------------------- the kernels' arithmetic on the CPU
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("level")), "host_level_check")
    subprocess.check_call(["g++"] + CHECK_FLAGS + [os.path.join(HERE, "host_level_check.cpp"), "-o", exe])
    return exe


def _run_check(exe, tmp_path, x, cases):
    """cases: (in_start, window, pairs, out_len) or, for a probe of stage_level alone, (in_start, window, pairs, out_len, flags,
    dtype, n_in); pairs: a list of (floor, peak).  Returns (outputs, stage records: one per case and pair)."""
    fin, fpairs, fcase, fout, fstage = (os.path.join(str(tmp_path), n) for n in ("in.bin", "pairs.bin", "case.bin", "out.bin", "stage.bin"))
    x.tofile(fin)
    all_pairs, recs = [], []
    for c in cases:
        flags, dtype, n_in = c[4:] if len(c) == 7 else (0, -1, 0)
        recs.append((c[0], c[1], c[3], len(all_pairs), len(c[2]), flags, dtype, n_in))
        all_pairs += [(float(fl), float(pk)) for fl, pk in c[2]]
    np.array(all_pairs, np.float64).reshape(-1, 2).tofile(fpairs)
    np.array(recs, dtype=np.int64).reshape(-1, 8).tofile(fcase)
    r = subprocess.run([exe, "u8" if x.dtype == np.uint8 else "f32", fin, fpairs, fcase, fout, fstage], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(fout, dtype=x.dtype), np.fromfile(fstage, dtype=np.int64).reshape(-1, 5)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("window", LC.WINDOWS)
def test_kernel_arithmetic_equals_level_host_bitwise(host_check, tmp_path, dtype, window):
    tile, most, lds = LC.launch_shape(dtype, window)
    assert most == 1024 and tile == (4096 if dtype == np.uint8 else 2048)
    for n_in in LC.ROWS:
        x = FC.samples(n_in, dtype, seed=n_in)
        cases = [(in_start, window, LC.PAIRS, out_len) for in_start in LC.starts(n_in) for out_len in LC.OUT_LENS]
        got, stages = _run_check(host_check, tmp_path, x, cases)
        want = []
        for in_start in LC.starts(n_in):
            # an output does not depend on how many follow it: the longest call, and the short ones on their own besides
            longest = {pair: LV.level_host(x, in_start, window, pair[0], pair[1], max(LC.OUT_LENS)) for pair in LC.PAIRS}
            for out_len in LC.OUT_LENS:
                for pair in LC.PAIRS:
                    want.append(longest[pair][:out_len])
                    if out_len <= 257:
                        assert LV.level_host(x, in_start, window, pair[0], pair[1], out_len).tobytes() == want[-1].tobytes()
        want = np.concatenate(want)
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), (n_in, int((got != want).sum()))
        out_lens = [c[3] for c in cases for _pair in LC.PAIRS]
        for out_len, (rc, t, n_tiles, grid, lds_bytes) in zip(out_lens, stages):
            assert rc == 0 and t == tile and n_tiles == -(-out_len // tile) and grid == min(n_tiles, most) and lds_bytes == lds
        if n_in == 70001 and window == 1:                     # at peak 0.75 both ends of the range are met
            assert want.min() == 0 and want.max() == (255 if dtype == np.uint8 else 1.0)


def test_hand_cases_and_the_pinned_order_by_the_header(host_check, tmp_path):
    for x, in_start, window, floor, peak, want in LC.hand_cases():
        got, _ = _run_check(host_check, tmp_path, x, [(in_start, window, [(floor, peak)], len(want))])
        assert got.tolist() == want, (x, window, peak)
    x, in_start, window, floor, peak = LC.order_case()
    got, _ = _run_check(host_check, tmp_path, x, [(in_start, window, [(floor, peak)], 1)])
    assert got.tolist() == [LC.ORDER_SEQUENTIAL]
    # what no stream holds, the arithmetic defines: a NaN or an infinite sample gives the centre wherever its window reaches
    x = np.array([0.25, np.nan, 0.75, np.inf, 0.75, 0.75, 0.75], np.float32)
    got, _ = _run_check(host_check, tmp_path, x, [(0, 3, [(1.0 / 128, 8.0)], 7)])
    want = LV.level_host(x, 0, 3, 1.0 / 128, 8.0, 7)
    assert got.tobytes() == want.tobytes() and got[:5].tolist() == [0.5] * 5 and got[5] > 0.5


def test_stage_level_refuses_what_the_entry_point_refuses(host_check, tmp_path):
    x = np.zeros(100, np.float32)
    ok = [(1.0 / 128, 8.0)]
    bad = [(s, w, [(fl, pk)], m, 0, -1, 0) for s, w, fl, pk, m in BAD] + [
        (0, 3, ok, 1, 1, -1, 0), (0, 3, ok, 1, 2, -1, 0), (0, 3, ok, 1, 3, -1, 0),      # a null pointer: the row, the output, both
        (0, 3, ok, 1, 0, 2, 0), (0, 3, ok, 1, 0, 7, 0),                                    # an unknown dtype
        (0, 3, ok, 1, 0, -1, -5), (0, 3, ok, 1, 0, -1, 1 << 62)]                           # n_in
    _got, stages = _run_check(host_check, tmp_path, x, bad)
    assert stages[:, 0].tolist() == [-1] * len(bad) and not stages[:, 1:].any()
    # float32 samples off their alignment: EALIGN, behind every other check
    off = [(0, 3, ok, 1, 4, -1, 0), (0, 3, ok, 1, 8, -1, 0), (0, 3, ok, 1, 12, -1, 0)]
    _got, stages = _run_check(host_check, tmp_path, x, off + [(0, 2, ok, 1, 4, -1, 0), (0, 3, ok, 1, 4, 0, 0)])
    assert stages[:, 0].tolist() == [-2, -2, -2, -1, 0]                    # (the last: uint8 samples lie anywhere)
    # the tile, the tile count, the grid and the LDS of short and long calls; several pairs of one case, a refused one among them
    f32 = lambda w: LC.launch_shape(np.float32, w)[2]
    u8 = LC.launch_shape(np.uint8, 1)[2]
    assert (f32(1), f32(129), f32(1023), u8) == (18424, 19576, 27624, 26912)
    fine = [(99, 1023, ok, (1 << 40) - 1, 0, 1, (1 << 62) - 1), (0, 1, ok, 1, 0, 1, 0), (0, 129, ok, 2049, 0, 1, 0),
            (0, 1023, ok, 1 << 30, 0, 0, 0), (0, 1, ok, 4097, 0, 0, 0),
            (0, 3, [(5e-324, 1e308), (np.nan, 1.0), (1.0, 1.0)], 2048 * 1024 + 1, 0, 1, 0)]
    _got, stages = _run_check(host_check, tmp_path, x, fine)
    assert stages.tolist() == [
        [0, 2048, 1 << 29, 1024, f32(1023)], [0, 2048, 1, 1, f32(1)], [0, 2048, 2, 2, f32(129)],
        [0, 4096, 1 << 18, 1024, u8], [0, 4096, 2, 2, u8],
        [0, 2048, 1025, 1024, f32(3)], [-1, 0, 0, 0, 0], [0, 2048, 1025, 1024, f32(3)]]


# ---------------------------------------------------------------------------------------------- the entry point's checks
def test_level_entry_point_validates_before_any_hip_call():
    """No pointer is dereferenced and no launch is made: every probe either fails a check (EINVAL) or, its arguments in range,
    stops at the alignment check behind them (EALIGN: float32 samples at an odd address)."""
    L = _native.lib()
    C = ctypes
    P, Q, ODD = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p((2 << 20) + 2)   # never dereferenced
    BIG = 1 << 50

    def call(n_in=1000, in_start=0, window=129, floor=1.0 / 128, peak=8.0, out_len=100, dtype=_native.F32, src=P, out=ODD):
        return L.sushi_hip_level(src, dtype, n_in, in_start, window, floor, peak, out, out_len, None)

    assert call() == -2 and call(src=C.c_void_p((1 << 20) + 1), out=Q) == -2
    for kw in ({"src": None}, {"out": None}, {"dtype": 2}, {"dtype": -1}, {"n_in": 0}, {"n_in": -5}, {"n_in": 1 << 62}, {"out_len": 0},
               {"out_len": -1}, {"out_len": 1 << 40}, {"in_start": -1}, {"in_start": 1000}, {"window": 0}, {"window": -3},
               {"window": 2}, {"window": 128}, {"window": 1024}, {"window": 1025}, {"floor": 0.0}, {"floor": -1.0},
               {"floor": float("inf")}, {"floor": float("nan")}, {"peak": 0.0}, {"peak": -8.0}, {"peak": float("inf")},
               {"peak": float("nan")}):
        assert call(**kw) == -1, kw
    # ... and the inclusive ends of every range pass the checks
    for kw in ({"n_in": 1}, {"in_start": 999}, {"window": 1}, {"window": 1023}, {"out_len": 1}, {"out_len": (1 << 40) - 1},
               {"n_in": BIG, "in_start": BIG - 1}, {"floor": 5e-324}, {"floor": 1.7e308}, {"peak": 5e-324}, {"peak": 1.7e308}):
        assert call(**kw) == -2, kw
    assert call(dtype=_native.U8, window=4) == -1 and call(dtype=_native.U8, out_len=0) == -1
    assert "sushi_hip_level" in _native.declared_symbols() and "sushi_hip_level_bytes" not in _native.declared_symbols()
    assert _native.ABI_VERSION == 13 and L.sushi_hip_abi_version() == 13


# ---------------------------------------------------------------------------------------------- WavStream.levelled, host path
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_levelled_on_the_host(monkeypatch, oracle, sample_type):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream, _locate
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    rate = 12000
    src = WavStream.from_samples(synth.make_dst_pcm(10, rate, seed=5), rate, sample_type=sample_type)
    pad, count = src.padding_size, src.sample_count
    for kw, (window, floor, peak) in (({}, (129, 1.0 / 128, 8.0)), ({"window": 33}, (33, 1.0 / 128, 8.0)),
                                      ({"window": 1023, "floor": 2.0 ** -20, "peak": 0.75}, (1023, 2.0 ** -20, 0.75))):
        f = src.levelled(**kw)
        assert (f.sample_rate, f.padding_size, f.sample_count) == (rate, pad, count)
        assert f.data.shape == src.data.shape and f.data.dtype == src.data.dtype and f._dev_row is None
        body = LV.level_host(src.data[0], pad, window, floor, peak, count)
        assert f.data[0, pad:pad + count].tobytes() == body.tobytes()
        assert (f.data[0, :pad] == body[0]).all() and (f.data[0, pad + count:] == body[-1]).all()
        assert f.duration_seconds == src.duration_seconds
    # the body's ends read the pads: a row whose pads differ from the body's edges gives other first and last samples
    f = src.levelled()
    odd = WavStream.from_prepared(src.data.copy(), rate, count, pad)
    odd.data[0, :pad] = odd.data[0, pad + 1000]
    odd.data[0, pad + count:] = odd.data[0, pad + 2000]
    g = odd.levelled()
    assert g.data[0, pad:pad + count].tobytes() == LV.level_host(odd.data[0], pad, 129, 1.0 / 128, 8.0, count).tobytes()
    assert g.data[0, pad + 64:pad + count - 64].tobytes() == f.data[0, pad + 64:pad + count - 64].tobytes()
    # a pattern cut from the result is an ordinary view of a live stream
    owner, off, length = _locate(f.get_substream(2.5, 4.5))
    assert owner is f and off == f.padding_size + int(rate * 2.5) and length == 2 * rate
    for bad in ({"window": 128}, {"window": 0}, {"window": 1025}, {"floor": 0.0}, {"floor": float("nan")}, {"peak": 0.0},
                {"peak": -1.0}, {"peak": float("inf")}):
        with pytest.raises(SushiError):
            src.levelled(**bad)
    # it composes: a band removed first, a levelled stream filtered, on another clock, and searched
    chain = src.filtered(low=150).levelled()
    assert chain.data[0, pad:pad + count].tobytes() == \
        LV.level_host(src.filtered(low=150).data[0], pad, 129, 1.0 / 128, 8.0, count).tobytes()
    assert f.filtered(low=150).sample_count == count and f.retimed("25/24").sample_count == ((count - 1) * 25) // 24 + 1
    evs = [(2.5, 4.5), (6.0, 7.0)]
    search = lambda row, pat: oracle.argmin_first(oracle.match_template_fft(row, pat, method=FC.SQ)[0])
    assert FC.found_shifts(f, *FC.requests(f, evs), search).tolist() == [0, 0]


# ---------------------------------------------------------------------------------------------- what levelling is for
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_levelling_gives_back_what_the_speech_hides(oracle, monkeypatch, sample_type):
    """Two mono dubs that share a bed under speech of their own, 14 dB above it (tests/level_cases.py): the plain search places at
    most 16 of 24 events at the planted shift, and every one of the 24 after levelled() on both streams."""
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    search = lambda row, pat: oracle.argmin_first(oracle.match_template_fft(row, pat, method=FC.SQ)[0])
    dst, src = LC.stream("dst", sample_type), LC.stream("src", sample_type)
    evs = LC.events()
    raw = FC.found_shifts(dst, *FC.requests(src, evs), search)
    l_dst, l_src = dst.levelled(), src.levelled()
    assert l_dst._dev_row is None                                       # level_host
    got = FC.found_shifts(l_dst, *FC.requests(l_src, evs), search)
    n_raw, n_levelled = int((raw == LC.OFFSET).sum()), int((got == LC.OFFSET).sum())
    print(sample_type, "plain", n_raw, "levelled", n_levelled)
    assert n_levelled == 24, got
    assert n_raw <= 16, raw
