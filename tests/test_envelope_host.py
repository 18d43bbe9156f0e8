"""Loudness contours without a GPU: the NumPy restatement of sushi_hip_envelope's arithmetic (sushi_amd/envelope.py), the kernel's
own arithmetic header compiled for the CPU (tests/host_envelope_check.cpp, a stand-alone program under AddressSanitizer + UBSan),
the entry point's argument checks, WavStream.envelope's host path, and what the contour is for: the scenarios of
tests/envelope_cases.py searched with the CPU oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import envelope_cases as EC
import host_checks
from sushi_amd import _native, envelope
from sushi_amd.common import SushiError

HERE = os.path.dirname(os.path.abspath(__file__))
CC = "ccoeff_normed"
SHAPES = [(1, 1), (2, 3), (8, 4), (7, 2), (64, 16), (256, 16), (256, 1)]          # (hop, span)
ROWS = [1, 5, 1000, 70001]


def _cases(n_in):
    """(in_start, hop, span, out_len) over every shape: in_start 0, 3 and n_in - 1 (both clamps act), an out_len that covers the
    row from in_start on and one that reads well past its end."""
    out = []
    for hop, span in SHAPES:
        for in_start in sorted({0, min(3, n_in - 1), n_in - 1}):
            cover = (n_in - in_start + hop - 1) // hop
            out.append((in_start, hop, span, cover))
            out.append((in_start, hop, span, cover + 2 * span + 37))
    return out


# ---------------------------------------------------------------------------------------------- envelope_host by hand
def test_uint8_hand_computed_cases():
    assert envelope.envelope_host(np.full(100, 128, np.uint8), 10, 8, 4, 20).tolist() == [0] * 20
    assert envelope.envelope_host(np.zeros(100, np.uint8), 0, 8, 4, 20).tolist() == [255] * 20       # 256 through the cap
    assert envelope.envelope_host(np.full(100, 255, np.uint8), 0, 8, 4, 5).tolist() == [254] * 5     # 2 * 127
    # W = 4: 2 E / W = E / 2.  E = 3 -> 1.5 -> 2;  E = 1 -> 0.5 -> 1;  E = 2 -> 1
    x = np.array([128, 129, 130, 128, 128, 127, 128, 128, 126, 128, 128, 128], np.uint8)
    assert envelope.envelope_host(x, 0, 4, 1, 3).tolist() == [2, 1, 1]
    # an odd W = 3: 2 E / 3.  E = 1 -> 0.67 -> 1;  E = 2 -> 1.33 -> 1;  E = 4 -> 2.67 -> 3
    x = np.array([128, 129, 128, 130, 128, 128, 132, 128, 128], np.uint8)
    assert envelope.envelope_host(x, 0, 3, 1, 3).tolist() == [1, 1, 3]
    # span 3: a = 1, output 0 sums blocks -1, 0, 1 and block -1 reads x[0] throughout; past the end the last sample holds
    x = np.array([138, 128, 128, 128, 148], np.uint8)
    #   blocks of hop 2 from in_start 0: B-1 = 20, B0 = 10, B1 = 0, B2 = 40 (x[4], x[4]), B3 = 40;  W = 6: (4 E + 6) // 12
    assert envelope.envelope_host(x, 0, 2, 3, 3).tolist() == [(4 * 30 + 6) // 12, (4 * 50 + 6) // 12, (4 * 80 + 6) // 12]


def test_float32_hand_computed_case():
    x = np.array([0.5, 1.0, 0.0, 0.75], np.float32)               # deviations 0, 0.5, 0.5, 0.25
    # hop 2, span 2 (a = 0): B0 = 0.5, B1 = 0.75, B2 = B3 = 0.5 (x[3] held);  E = 1.25, 1.25, 1.0;  2 E / 4
    out = envelope.envelope_host(x, 0, 2, 2, 3)
    assert out.dtype == np.float32 and out.tolist() == [0.625, 0.625, 0.5]
    # span 3 (a = 1): B-1 = 0 (x[0] twice);  E0 = 0 + 0.5 + 0.75;  2 E / 6
    assert envelope.envelope_host(x, 0, 2, 3, 1)[0] == np.float32(2.5 / 6.0)
    assert envelope.envelope_host(np.full(50, 0.5, np.float32), 7, 1, 1, 60).tolist() == [0.0] * 60
    assert envelope.envelope_host(np.array([0.0, 1.0], np.float32), 0, 1, 1, 2).tolist() == [1.0, 1.0]   # full scale gives 1


def _pairwise(v):
    return v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:])


def test_float32_sum_order_is_pinned():
    x = EC.order_case()
    d = [abs(float(v) - 0.5) for v in x]
    assert d == [2.0 ** 31 + 0.5, 127.5, 3 * 2.0 ** -24, 3 * 2.0 ** -24]                       # the samples hold them exactly
    seq = ((0.0 + d[0]) + d[1]) + d[2] + d[3]
    pair = _pairwise(d)
    assert seq != pair and np.float32((seq + seq) / 4.0) == 2.0 ** 30 and np.float32((pair + pair) / 4.0) == 2.0 ** 30 + 128
    assert envelope.envelope_host(x, 0, 4, 1, 1)[0] == np.float32(2.0 ** 30)                    # the block sum's order
    assert envelope.envelope_host(x, 1, 1, 4, 1)[0] == np.float32(2.0 ** 30)                    # the window sum's (a = 1: blocks -1 .. 2)


def test_envelope_host_refuses_bad_arguments():
    x = np.zeros(100, np.uint8)
    for bad in ((0, 0, 1, 1), (0, 257, 1, 1), (0, 1, 0, 1), (0, 1, 65, 1), (0, 256, 17, 1), (0, 128, 33, 1), (-1, 8, 4, 1),
                (100, 8, 4, 1), (0, 8, 4, 0), (0, 8, 4, 1 << 40)):
        with pytest.raises(SushiError):
            envelope.envelope_host(x, *bad)
    with pytest.raises(SushiError):
        envelope.envelope_host(np.zeros(10, np.int16), 0, 8, 4, 1)
    with pytest.raises(SushiError):
        envelope.envelope_host(np.zeros((1, 10), np.uint8), 0, 8, 4, 1)
    assert envelope.envelope_host(x, 99, 256, 16, 1).shape == (1,) and envelope.envelope_host(x, 0, 64, 64, 2).shape == (2,)


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic on the CPU
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("envelope")), "host_envelope_check")
    subprocess.check_call(["g++"] + host_checks.KERNEL_ARITHMETIC + [os.path.join(HERE, "host_envelope_check.cpp"), "-o", exe])
    return exe


def _run_check(exe, tmp_path, x, cases):
    fin, fcase, fout, fstage = (os.path.join(str(tmp_path), n) for n in ("in.bin", "case.bin", "out.bin", "stage.bin"))
    x.tofile(fin)
    np.array(cases, dtype=np.int64).reshape(-1, 4).tofile(fcase)
    r = subprocess.run([exe, "u8" if x.dtype == np.uint8 else "f32", fin, fcase, fout, fstage], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(fout, dtype=x.dtype), np.fromfile(fstage, dtype=np.int64).reshape(-1, 4)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_kernel_arithmetic_equals_envelope_host_bitwise(host_check, tmp_path, dtype):
    for n_in in ROWS:
        x = EC.samples(n_in, dtype, seed=n_in)
        cases = _cases(n_in)
        got, stages = _run_check(host_check, tmp_path, x, cases)
        want = np.concatenate([envelope.envelope_host(x, *c) for c in cases])
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), n_in
        for (in_start, hop, span, out_len), (rc, tile, n_tiles, grid) in zip(cases, stages):
            assert rc == 0 and tile == min(4096 // hop, 512) and n_tiles == -(-out_len // tile) and grid == min(n_tiles, 1024)
    # the hand-computed cases and the pinned order, by the header's own code
    if dtype == np.uint8:
        got, _ = _run_check(host_check, tmp_path, np.array([128, 129, 130, 128, 128, 127, 128, 128, 126, 128, 128, 128], np.uint8),
                            [(0, 4, 1, 3)])
        assert got.tolist() == [2, 1, 1]
        got, _ = _run_check(host_check, tmp_path, np.zeros(64, np.uint8), [(0, 8, 4, 6)])
        assert got.tolist() == [255] * 6
    else:
        got, _ = _run_check(host_check, tmp_path, EC.order_case(), [(0, 4, 1, 1), (1, 1, 4, 1)])
        assert got.tolist() == [2.0 ** 30, 2.0 ** 30]
        got, _ = _run_check(host_check, tmp_path, np.array([0.5, 1.0, 0.0, 0.75], np.float32), [(0, 2, 2, 3), (0, 2, 3, 1)])
        assert got.tolist() == [0.625, 0.625, 0.5, float(np.float32(2.5 / 6.0))]


def test_stage_envelope_refuses_what_the_entry_point_refuses(host_check, tmp_path):
    x = np.zeros(1000, np.uint8)
    bad = [(0, 0, 1, 1), (0, 257, 1, 1), (0, 1, 0, 1), (0, 1, 65, 1), (0, 256, 17, 1), (-1, 8, 4, 1), (1000, 8, 4, 1), (0, 8, 4, 0),
           (0, 8, 4, 1 << 40)]
    got, stages = _run_check(host_check, tmp_path, x, bad + [(999, 256, 16, 3)])
    assert stages[:-1, 0].tolist() == [-1] * len(bad) and stages[-1].tolist() == [0, 16, 1, 1] and got.shape == (3,)


# ---------------------------------------------------------------------------------------------- the entry point's checks
def test_envelope_entry_point_validates_before_any_hip_call():
    """No pointer is dereferenced and no launch is made: every probe either fails a check (EINVAL) or, its arguments in range,
    stops at the alignment check behind them (EALIGN: float32 samples at an odd address)."""
    L = _native.lib()
    C = ctypes
    P, Q, ODD = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p((2 << 20) + 2)               # never dereferenced
    BIG = 1 << 50

    def call(n_in=1000, in_start=0, hop=8, span=4, out_len=100, dtype=_native.F32, src=P, out=ODD):
        return L.sushi_hip_envelope(src, dtype, n_in, in_start, hop, span, out, out_len, None)

    assert call() == -2 and call(src=C.c_void_p((1 << 20) + 1), out=Q) == -2
    for kw in ({"src": None}, {"out": None}, {"dtype": 2}, {"dtype": -1}, {"n_in": 0}, {"n_in": -5}, {"out_len": 0}, {"out_len": -1},
               {"out_len": 1 << 40}, {"in_start": -1}, {"in_start": 1000}, {"hop": 0}, {"hop": -8}, {"hop": 257}, {"span": 0},
               {"span": 65}, {"hop": 256, "span": 17}, {"hop": 128, "span": 33}, {"hop": 65, "span": 64}, {"n_in": 1 << 62}):
        assert call(**kw) == -1, kw
    # ... and the inclusive ends of every range pass the checks
    for kw in ({"n_in": 1}, {"in_start": 999}, {"hop": 1, "span": 1}, {"hop": 1, "span": 64}, {"hop": 256, "span": 16},
               {"hop": 64, "span": 64}, {"out_len": 1}, {"out_len": (1 << 40) - 1}, {"n_in": BIG, "in_start": BIG - 1},
               {"out_len": 5000}):
        assert call(**kw) == -2, kw
    # uint8 samples have no alignment to miss: only the argument checks are probed
    assert call(dtype=_native.U8, hop=0) == -1 and call(dtype=_native.U8, out_len=0) == -1
    assert "sushi_hip_envelope" in _native.declared_symbols() and "sushi_hip_envelope_bytes" not in _native.declared_symbols()


# ---------------------------------------------------------------------------------------------- WavStream.envelope, host path
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_envelope_on_the_host(monkeypatch, sample_type):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream, _locate
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    rate = 12000
    src = WavStream.from_samples(synth.make_dst_pcm(20, rate, seed=5), rate, sample_type=sample_type)
    pad, count = src.padding_size, src.sample_count
    for hop, span in ((8, 4), (16, 3), (1, 1)):
        env = src.envelope(hop, span)
        n_new, new_pad = -(-count // hop), pad // hop
        assert (env.sample_rate, env.padding_size, env.sample_count) == (rate // hop, new_pad, n_new)
        assert env.data.shape == (1, 2 * new_pad + n_new) and env.data.dtype == src.data.dtype
        body = envelope.envelope_host(src.data[0], pad, hop, span, n_new)
        assert env.data[0, new_pad:new_pad + n_new].tobytes() == body.tobytes()
        assert (env.data[0, :new_pad] == body[0]).all() and (env.data[0, new_pad + n_new:] == body[-1]).all()
        assert abs(env.duration_seconds - src.duration_seconds) < hop / float(rate)
    assert src.envelope().data.tobytes() == src.envelope(8, 4).data.tobytes()
    # a pattern cut from the result is an ordinary view of a live stream
    env = src.envelope()
    owner, off, length = _locate(env.get_substream(7.5, 9.5))
    assert owner is env and off == env.padding_size + int(1500 * 7.5) and length == 3000
    # hop must divide the rate
    for bad in (7, 9, 0, 257):
        with pytest.raises(SushiError):
            src.envelope(bad, 2)
    with pytest.raises(SushiError):
        src.envelope(8, 65)
    # an all-centre row has no contour
    centre = 128 if sample_type == "uint8" else 0.5
    flat = WavStream.from_prepared(np.full((1, 2 * 1200 + 5000), centre, src.data.dtype), 12000, 5000, 1200)
    e = flat.envelope(1, 1)
    assert (e.sample_rate, e.padding_size, e.sample_count) == (12000, 1200, 5000) and not e.data.any()
    # a 44.1 kHz file at 12 kHz: the pad is ten seconds of the FILE's frames, 441000 samples; hop 16 leaves 27562 (and a half)
    cd = WavStream.from_prepared(np.full((1, 2 * 441000 + 12005), centre, src.data.dtype), 12000, 12005, 441000)
    e = cd.envelope(16, 4)
    assert (e.sample_rate, e.padding_size, e.sample_count) == (750, 27562, 751)
    assert e.data.shape == (1, 2 * 27562 + 751) and not e.data.any()
    cd.sample_rate = 44100
    with pytest.raises(SushiError):
        cd.envelope(16, 4)                                               # 44100 = 16 * 2756.25


# ---------------------------------------------------------------------------------------------- what the contour is for
def _oracle_search(oracle):
    return lambda row, pat: oracle.argmax_first(oracle.match_template_fft(row, pat, method=CC)[0])


@pytest.fixture(scope="module")
def host_streams():
    """{(name, sample type): (stream, its contour)} on the host path, made once."""
    made = {}
    old = os.environ.get("SUSHI_HIP_LOAD")
    os.environ["SUSHI_HIP_LOAD"] = "host"
    try:
        for st in ("uint8", "float32"):
            for name in ("dst",) + EC.CASES + ("speed",):
                s = EC.stream(name, st)
                made[(name, st)] = (s, s.envelope(EC.HOP, EC.SPAN))
    finally:
        if old is None:
            del os.environ["SUSHI_HIP_LOAD"]
        else:
            os.environ["SUSHI_HIP_LOAD"] = old
    return made


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_contour_search_places_every_event_where_the_waveform_search_cannot(oracle, host_streams, sample_type):
    """hop 8 / span 4: 24 of 24 events within +-1 contour sample of 3.7 s in all three cases; the plain waveform search places
    fewer than 3 of 24 within +-hop samples where the polarity or the carrier differs (measured: 0), and all 24 in the control."""
    search = _oracle_search(oracle)
    dst, dst_env = host_streams[("dst", sample_type)]
    evs = EC.events()
    true_env = EC.OFFSET // EC.HOP
    assert true_env * EC.HOP == EC.OFFSET
    for name in EC.CASES:
        src, src_env = host_streams[(name, sample_type)]
        got = EC.found_shifts(dst_env, *EC.requests(src_env, dst_env, evs), search)
        hits = int((np.abs(got - true_env) <= 1).sum())
        print(sample_type, name, "contour", hits)
        assert hits == 24, (name, got)
        wave = EC.found_shifts(dst, *EC.requests(src, dst, evs), search)
        near = int((np.abs(wave - EC.OFFSET) <= EC.HOP).sum())
        print(sample_type, name, "waveform", near)
        assert near == 24 if name == "same" else near < 3, (name, near)


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_contour_of_a_sped_up_source_retimed(oracle, host_streams, monkeypatch, sample_type):
    """A 25/24 source with a carrier of its own, through envelope().retimed('25/24'): 24 of 24 events within +-2 contour samples
    of where the event lies on the destination's clock."""
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    search = _oracle_search(oracle)
    _dst, dst_env = host_streams[("dst", sample_type)]
    _src, src_env = host_streams[("speed", sample_type)]
    retimed = src_env.retimed(EC.SPEED)
    evs = EC.events(EC.SPEED)
    pats, centres, starts = EC.requests(retimed, dst_env, evs, scale=float(EC.SPEED))
    where = EC.found_shifts(dst_env, pats, centres, starts, search) + starts
    true = np.array([s * float(EC.SPEED) * EC.RATE / EC.HOP for s, _e in evs])
    hits = int((np.abs(where - true) <= 2).sum())
    print(sample_type, "speed", hits)
    assert hits == 24, where - true
