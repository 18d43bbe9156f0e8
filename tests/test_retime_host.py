"""Retiming without a GPU: the NumPy restatement of sushi_hip_retime's arithmetic (sushi_amd/retime.py), the kernel's own
arithmetic header compiled for the CPU (tests/host_retime_check.cpp, under AddressSanitizer + UBSan), the entry point's argument
checks, and what rests on them: as_ratio, choose_speed, fit_speed, WavStream.retimed's host path, calculate_shifts_at_speed."""
import ctypes
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from host_checks import build_check
from sushi_amd import _native, retime, synth
from sushi_amd.common import SushiError

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
STEPS = [(24, 25), (25, 24), (1001, 960), (960, 1001), (1, 8), (8, 1), (1048575, 1048576)]      # (num, den): input samples per output


def _samples(n, dtype, seed=0):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    return rng.random(n, dtype=np.float32)


def _longest(n_in, in_start, num, den):
    """Most outputs a segment from in_start can have: the last read (out_len - 1) * num // den stays at or below n_in - 1."""
    return ((n_in - 1 - in_start + 1) * den - 1) // num + 1


# ---------------------------------------------------------------------------------------------- retime_host
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_step_one_is_identity(dtype):
    x = _samples(5000, dtype)
    out = retime.retime_host(x, [(0, 0, 5000, 1, 1)])
    assert out.dtype == x.dtype and out.tobytes() == x.tobytes()
    part = retime.retime_host(x, [(100, 7, 300, 3, 3)])                 # 3 / 3 is a step of one too: r is always 0
    assert part.shape == (307,) and part[7:].tobytes() == x[100:400].tobytes() and not part[:7].any()


def test_hand_computed_case_rounds_half_up():
    x = np.array([0, 255, 10], np.uint8)
    out = retime.retime_host(x, [(0, 0, 5, 1, 2)])
    assert out.tolist() == [0, 128, 255, 133, 10]                        # 127.5 -> 128, 132.5 -> 133
    f = retime.retime_host(x.astype(np.float32), [(0, 0, 5, 1, 2)])
    assert f.tolist() == [0.0, 127.5, 255.0, 132.5, 10.0]


def test_last_read_is_clamped():
    """The last output sits exactly on the last input sample (r == 0 at j = n_in - 1): its neighbour j + 1 is clamped, not read."""
    x = _samples(101, np.uint8, seed=1)
    out = retime.retime_host(x, [(0, 0, 201, 1, 2)])
    assert out[-1] == x[-1] and out[0] == x[0] and (out[::2] == x).all()
    # behind the last sample the edge value holds: j = n_in - 1 with r > 0 reads x[n_in - 1] twice
    out = retime.retime_host(x, [(99, 0, 4, 1, 2)])
    assert out[2] == x[100] and out[3] == x[100]
    with pytest.raises(SushiError):
        retime.retime_host(x, [(0, 0, 203, 1, 2)])                       # a last read at j = n_in
    with pytest.raises(SushiError):
        retime.retime_host(x, [(0, 0, 10, 9, 1)])
    with pytest.raises(SushiError):
        retime.retime_host(x, [(0, 0, 10, 1, (1 << 20) + 1)])
    with pytest.raises(SushiError):
        retime.retime_host(x, [(0, 5, 10, 1, 1)], out=np.zeros(14, np.uint8))


def test_index_arithmetic_is_64_bit():
    """out_len = 300000 at 25025 / 24000: i * num passes 2^32.  Against the same operations on Python's integers and floats."""
    num, den, out_len = 25025, 24000, 300000
    n_in = (out_len - 1) * num // den + 2
    for dtype in (np.uint8, np.float32):
        x = _samples(n_in, dtype, seed=2)
        out = retime.retime_host(x, [(0, 0, out_len, num, den)])
        assert (out_len - 1) * num > 1 << 32
        for i in list(range(0, out_len, 9973)) + list(range(out_len - 2000, out_len)):
            t = i * num
            j, r = t // den, t % den
            a, b = float(x[j]), float(x[min(j + 1, n_in - 1)])
            y = a + (r / den) * (b - a)
            want = np.uint8(int(y + 0.5)) if dtype == np.uint8 else np.float32(y)
            assert out[i] == want, (i, out[i], want)


# ---------------------------------------------------------------------------------------------- as_ratio, choose_speed, fit_speed
def test_as_ratio_forms_and_rejections():
    assert retime.as_ratio(Fraction(25, 24)) == Fraction(25, 24)
    assert retime.as_ratio(1) == Fraction(1) and retime.as_ratio(2) == 2
    assert retime.as_ratio("25/24") == Fraction(25, 24) and retime.as_ratio(" 1001 / 960 ") == Fraction(1001, 960)
    assert retime.as_ratio(25 / 24) == Fraction(25, 24) and retime.as_ratio(1001 / 1000) == Fraction(1001, 1000)
    assert retime.as_ratio(24000 / 1001 / 25) == Fraction(960, 1001)
    assert retime.as_ratio(8) == 8 and retime.as_ratio("1/8") == Fraction(1, 8)
    assert retime.as_ratio(Fraction(1 << 20, (1 << 20) - 1)).numerator == 1 << 20
    for bad in (0, -1, "9", "1/9", Fraction(81, 10), Fraction((1 << 20) + 1, 1 << 20), Fraction(1 << 19, (1 << 20) + 1), "x", "1/0",
                None, True, 0.0, [1]):
        with pytest.raises(SushiError):
            retime.as_ratio(bad)
    assert retime.STANDARD_SPEEDS == (1, Fraction(25, 24), Fraction(24, 25), Fraction(1001, 960), Fraction(960, 1001),
                                      Fraction(1001, 1000), Fraction(1000, 1001))
    assert all(isinstance(s, Fraction) for s in retime.STANDARD_SPEEDS)
    # speed s: the source is read at 1 / s
    assert retime.speed_segment("25/24", 5, 6, 7) == (5, 6, 7, 24, 25)


def test_choose_speed_clear_and_ambiguous():
    cands = [1, "25/24", "1001/1000"]
    speed, scores = retime.choose_speed(cands, [[0.40, 0.38, 0.41, 0.39], [0.006, 0.007, 0.30, 0.005], [0.26, 0.27, 0.25, 0.28]])
    assert speed == Fraction(25, 24)                                     # one probe that missed does not move the median
    assert np.allclose(scores, [0.395, 0.0065, 0.265])
    speed, scores = retime.choose_speed(cands, [[0.40] * 4, [0.3 * 0.26] * 4, [0.26] * 4])
    assert speed is None and int(np.argmin(scores)) == 1                 # 0.3 x the runner-up: not clear enough
    speed, _ = retime.choose_speed(cands, [[0.40] * 4, [0.25 * 0.26] * 4, [0.26] * 4])
    assert speed == Fraction(25, 24)                                     # at 0.25 x it is
    assert retime.choose_speed([1], [[0.001]])[0] is None                # nothing to hold it against
    speed, scores = retime.choose_speed([1, 2], [[0.01, np.nan], [np.nan, 0.5]])
    assert speed == 1 and scores.tolist() == [0.01, 0.5]


def test_fit_speed_recovers_the_slope():
    src = np.array([100000, 460000, 820000, 1180000], np.int64)
    dst = 60000 + src * 1001 // 960                                       # exact positions, floored to samples
    got = retime.fit_speed(src, dst)
    assert abs(got - 1001 / 960) <= 1.0 / 360000                          # an index is off by < 1 sample over >= 360000
    dst_bad = dst.copy()
    dst_bad[2] += 500000                                                  # one probe matched somewhere else
    assert abs(retime.fit_speed(src, dst_bad) - 1001 / 960) <= 1.0 / 360000
    with pytest.raises(SushiError):
        retime.fit_speed([5, 5], [1, 2])


# ---------------------------------------------------------------------------------------------- the entry point's checks
def _seg(*rows):
    return np.array([r.tolist() if isinstance(r, np.void) else tuple(r) for r in rows], dtype=_native.RETIME_SEGMENT_DTYPE)


def test_retime_entry_point_validates_before_any_hip_call():
    L = _native.lib()
    C = ctypes
    assert L.sushi_hip_retime_bytes(0) == 0 and L.sushi_hip_retime_bytes(-3) == 0
    assert L.sushi_hip_retime_bytes(1) == 256 and L.sushi_hip_retime_bytes(23) % 256 == 0
    assert L.sushi_hip_retime_bytes(23) >= 23 * 32
    P, Q, M = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)            # never dereferenced
    BIG = 1 << 50

    def call(seg, dtype=_native.U8, n_in=1000, n_out=1000, src=P, out=Q, mem=M, mem_bytes=0, n_seg=None, seg_ptr="own"):
        return L.sushi_hip_retime(src, dtype, n_in, seg.ctypes.data if seg_ptr == "own" else seg_ptr,
                                  seg.shape[0] if n_seg is None else n_seg, out, n_out, mem, mem_bytes, None)

    ok = _seg((0, 0, 100, 25, 24))
    # a call that passes every check but the workspace's size ends with ENOSPACE: what is valid is told apart from what is not
    assert call(ok) == -4
    assert call(ok, mem_bytes=L.sushi_hip_retime_bytes(1) - 1) == -4
    assert call(ok, mem=C.c_void_p((3 << 20) + 8), mem_bytes=1 << 20) == -2
    assert call(ok, mem=C.c_void_p((3 << 20) + 128), mem_bytes=1 << 20) == -2
    for kw in ({"src": None}, {"out": None}, {"mem": None}, {"seg_ptr": None}):
        assert call(ok, mem_bytes=1 << 20, **kw) == -1, kw
    assert call(ok, dtype=2) == -1 and call(ok, dtype=-1) == -1
    assert call(ok, n_seg=0) == -1 and call(ok, n_seg=-1) == -1
    for bad in ((0, 0, 100, 0, 24), (0, 0, 100, 25, 0), (0, 0, 100, -1, 1), (0, 0, 100, (1 << 20) + 1, 1 << 20),
                (0, 0, 100, 1 << 20, (1 << 20) + 1),              # num, den in [1, 2^20]
                (0, 0, 10, 9, 1), (0, 0, 10, 1, 9), (0, 0, 10, 8001, 1000),   # num / den in [1/8, 8]
                (0, 0, 0, 1, 1), (0, 0, -5, 1, 1),                            # out_len >= 1
                (-1, 0, 10, 1, 1), (1000, 0, 1, 1, 1),                        # in_start inside the input
                (0, 0, 1001, 1, 1), (500, 0, 1001, 1, 2), (999, 0, 2, 1, 1),   # the last read
                (0, -1, 10, 1, 1), (0, 991, 10, 1, 1), (0, 1000, 1, 1, 1)):    # outputs inside [0, n_out)
        assert call(_seg(bad), mem_bytes=1 << 20) == -1, bad
        assert call(_seg(ok[0], bad), mem_bytes=1 << 20) == -1, bad                    # every segment is checked
    assert call(_seg((0, 0, 1 << 40, 1, 1)), n_in=BIG, n_out=BIG, mem_bytes=1 << 20) == -1
    # ... and the inclusive ends of every range pass the checks
    for good in ((0, 0, 10, 8, 1), (0, 0, 10, 1, 8), (0, 0, 10, 1 << 20, 1 << 20), (0, 0, 1000, 1, 1), (500, 0, 999, 1, 2),
                 (999, 0, 1, 1, 1), (999, 0, 8, 1, 8), (0, 990, 10, 1, 1), (0, 999, 1, 1, 1)):
        assert call(_seg(good)) == -4, good
    assert call(_seg((0, 0, (1 << 40) - 1, 1, 1)), n_in=BIG, n_out=BIG) == -4
    assert call(_seg((BIG - 1, BIG - 1, 1, 1, 1)), n_in=BIG, n_out=BIG) == -4
    assert call(ok, n_in=0) == -1 and call(ok, n_out=0) == -1
    # float32 samples are 4-byte aligned
    assert call(ok, dtype=_native.F32, out=C.c_void_p((2 << 20) + 2), mem_bytes=1 << 20) == -2
    assert call(ok, dtype=_native.F32) == -4


def test_retime_segment_layout_matches_header(tmp_path):
    src, exe = os.path.join(tmp_path, "layout.c"), os.path.join(tmp_path, "layout")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include <stddef.h>\n#include "sushi_hip.h"\n'
                'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(SushiHipRetimeSegment),'
                'offsetof(SushiHipRetimeSegment,in_start),offsetof(SushiHipRetimeSegment,out_off),'
                'offsetof(SushiHipRetimeSegment,out_len),offsetof(SushiHipRetimeSegment,num),'
                'offsetof(SushiHipRetimeSegment,den));return 0;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe])     # the header is plain C
    vals = [int(v) for v in subprocess.check_output([exe]).split()]
    d = _native.RETIME_SEGMENT_DTYPE
    assert vals == [32, 0, 8, 16, 24, 28]
    assert vals == [d.itemsize] + [d.fields[k][1] for k in ("in_start", "out_off", "out_len", "num", "den")]


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic on the CPU
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return build_check("host_retime_check", tmp_path_factory.mktemp("retime"))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_kernel_arithmetic_equals_retime_host_bitwise(host_check, tmp_path, dtype):
    n_in = 20011
    x = _samples(n_in, dtype, seed=3)
    segs, off = [], 3
    for k, (num, den) in enumerate(STEPS):
        in_start = 17 * k
        out_len = min(_longest(n_in, in_start, num, den), 40000 + k)      # as far as the input goes (the last read: n_in - 1 or just below)
        segs.append((in_start, off, out_len, num, den))
        off += out_len + 5
        segs.append((n_in - 1 - 3 * k, off, 1 + k % 2, num, den))           # short ones at the input's end
        off += 7
    segs.append((n_in - 1, off, 1, 1, 1))
    n_out = off + 4
    want = retime.retime_host(x, segs, out=np.zeros(n_out, dtype))
    assert any(s[0] + (s[2] - 1) * s[3] // s[4] == n_in - 1 for s in segs)
    fin, fseg, fout = (os.path.join(tmp_path, n) for n in ("in.bin", "seg.bin", "out.bin"))
    x.tofile(fin)
    np.array(segs, dtype=_native.RETIME_SEGMENT_DTYPE).tofile(fseg)
    r = subprocess.run([host_check, "u8" if dtype == np.uint8 else "f32", fin, fseg, fout, str(n_out)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(fout, dtype=dtype)
    assert got.shape == want.shape and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- WavStream.retimed, host path
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_retimed_on_the_host(monkeypatch, sample_type):
    from sushi_amd.wav import WavStream, _locate
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    rate = 12000
    src = WavStream.from_samples(synth.make_dst_pcm(20, rate, seed=5), rate, sample_type=sample_type)
    same = src.retimed(1)
    assert same is not src and same.data is not src.data
    assert same.data.dtype == src.data.dtype and same.data.tobytes() == src.data.tobytes()
    assert (same.sample_count, same.padding_size, same.sample_rate) == (src.sample_count, src.padding_size, src.sample_rate)
    speed = Fraction(25, 24)
    r = src.retimed("25/24")
    n_new = (src.sample_count - 1) * 25 // 24 + 1
    pad = src.padding_size
    assert r.sample_count == n_new and r.padding_size == pad and r.sample_rate == rate
    assert r.data.shape == (1, 2 * pad + n_new) and r.data.dtype == src.data.dtype
    body = retime.retime_host(src.data[0], [(pad, 0, n_new, 24, 25)])
    assert r.data[0, pad:pad + n_new].tobytes() == body.tobytes()
    assert (r.data[0, :pad] == body[0]).all() and (r.data[0, pad + n_new:] == body[-1]).all()
    assert abs(r.duration_seconds - src.duration_seconds * 25 / 24) <= 1.0 / rate
    # a pattern cut from the result is an ordinary view of a live stream
    t = 7.3
    view = r.get_substream(t * float(speed), (t + 2.0) * float(speed))
    owner, off, length = _locate(view)
    assert owner is r and off == pad + int(rate * t * float(speed)) and length == view.shape[1] > 2 * rate
    # the source instant t lies at t * speed: sample k of the source is sample k * 25 / 24 of the result
    k = 24 * 1000
    assert r.data[0, pad + k * 25 // 24] == src.data[0, pad + k]
    slow = src.retimed(Fraction(960, 1001))
    assert slow.sample_count == (src.sample_count - 1) * 960 // 1001 + 1
    with pytest.raises(SushiError):
        src.retimed(9)


# ---------------------------------------------------------------------------------------------- calculate_shifts_at_speed
def test_shifts_at_speed_one_equals_the_plain_function():
    """Shadow events, the unmodified state machine, results copied back -- links included (groups past the destination's end)."""
    from shifts_fakes import SCENARIOS, FakeDestination, FakeSource
    from sushi_amd.shifts import ScriptEvent, calculate_shifts, calculate_shifts_at_speed

    class Source(FakeSource):
        def retimed(self, speed):
            assert speed == 1
            return self

    for sc in SCENARIOS:
        if sc["name"] not in ("past-end", "steps", "groups-of-three"):
            continue
        size = sc.get("group_size", 1)
        runs = []
        for at_speed in (False, True):
            events = [ScriptEvent(s, s + sc["length"]) for s in sc["starts"]]
            groups = [events[k:k + size] for k in range(0, len(events), size)]
            src, dst = Source(sc["script"]["sample_rate"], sc["script"]["duration"] + 60), FakeDestination(sc["script"])
            if at_speed:
                calculate_shifts_at_speed(src, dst, groups, 1, sc["window"], sc["max_window"], sc["rewind"], batched=False)
            else:
                calculate_shifts(src, dst, groups, sc["window"], sc["max_window"], sc["rewind"])
            runs.append((events, dst.calls))
        (plain, calls0), (shadowed, calls1) = runs
        assert calls0 == calls1
        assert [(e.shift, e.diff, e.linked) for e in plain] == [(e.shift, e.diff, e.linked) for e in shadowed]
        for a, b in zip(plain, shadowed):
            if a.linked:
                assert plain.index(a._linked_event) == shadowed.index(b._linked_event)
        if sc["name"] == "past-end":
            assert any(e.linked for e in shadowed)
