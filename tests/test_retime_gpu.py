"""Retiming on the GPU: sushi_hip_retime against its NumPy restatement (bit for bit), WavStream.retimed's two paths, and the job it
is for -- a source that plays at another speed than the destination: estimate_speed names the speed, patterns cut from the
retimed source are found where they lie, calculate_shifts_at_speed carries events across."""
import math
from fractions import Fraction

import numpy as np
import pytest

from sushi_amd import retime, synth

pytestmark = pytest.mark.gpu

RATE = 12000
OFFSET_S = 5.0
STEPS = [(24, 25), (25, 24), (1001, 960), (960, 1001), (1, 8), (8, 1), (1048575, 1048576)]      # (num, den): input samples per output
SENTINEL = {np.dtype(np.uint8): np.uint8(0xA5), np.dtype(np.float32): np.float32(-7.25)}


def _samples(n, dtype, seed=0):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    return rng.random(n, dtype=np.float32)


def _run_device(x, segs, n_out):
    import torch
    out = torch.full((n_out,), SENTINEL[x.dtype].item(), dtype=torch.uint8 if x.dtype == np.uint8 else torch.float32, device="cuda")
    got = retime.retime_device(torch.from_numpy(x).cuda(), segs, out=out)
    assert got is out
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_many_segments_in_one_launch(dtype):
    """23 segments in one launch: every step of the list at out_len 1, 63, 64, 65 and 4097, output offsets that are no multiples
    of 16 (every phase of the 16-byte store grid), one segment of 300000 outputs at 25025 / 24000 (i * num passes 2^32) and one
    whose last read is exactly the last input sample.  (The input has 320000 samples, not 200000: 300000 outputs at 25025 / 24000
    read 312813 of them.)  Bitwise against retime_host; what lies between the segments keeps its sentinel."""
    n_in = 320000
    x = _samples(n_in, dtype, seed=11)
    lens = [1, 63, 64, 65, 4097]
    segs, off, k = [], 1, 0
    for num, den in STEPS:
        for _ in range(3):
            out_len = lens[k % len(lens)]
            in_start = (7919 * k) % (n_in - 8 * 4097 - 1)
            segs.append((in_start, off, out_len, num, den))
            off += out_len + 1 + k % 7
            if off % 16 == 0:
                off += 3
            k += 1
    segs.append((1000, off, 300000, 25025, 24000))
    off += 300000 + 5
    segs.append((n_in - 1 - 4096 * 24 // 25, off, 4097, 24, 25))
    n_out = off + 4097 + 9
    assert len(segs) == 23 and all(s[1] % 16 for s in segs)
    assert segs[-1][0] + (4097 - 1) * 24 // 25 == n_in - 1
    assert len({s[1] % 16 for s in segs}) >= 8 and len({s[1] % 4 for s in segs}) == 4
    want = retime.retime_host(x, segs, out=np.full(n_out, SENTINEL[x.dtype], dtype))
    got = _run_device(x, segs, n_out)
    covered = np.zeros(n_out, bool)
    for _, o, m, _, _ in segs:
        covered[o:o + m] = True
    assert covered.sum() == sum(s[2] for s in segs) and not covered.all()
    assert got[~covered].tobytes() == np.full(int((~covered).sum()), SENTINEL[x.dtype], dtype).tobytes()
    for in_start, o, m, num, den in segs:
        assert got[o:o + m].tobytes() == want[o:o + m].tobytes(), (in_start, o, m, num, den)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("dtype,out_len", [(np.uint8, 3000000), (np.float32, 3000000), (np.uint8, 8500000), (np.float32, 4500000)])
def test_one_long_segment(dtype, out_len):
    """One segment of 3000000 outputs; and of enough outputs that the grid strides over its tiles more than once (2048 workgroups
    of 256 threads, 16 uint8 / 8 float32 outputs a thread)."""
    num, den = 24, 25
    n_in = (out_len - 1) * num // den + 1                                  # the last read is the last input sample
    x = _samples(n_in, dtype, seed=12)
    seg = [(0, 5, out_len, num, den)]
    want = retime.retime_host(x, seg, out=np.full(out_len + 11, SENTINEL[x.dtype], dtype))
    got = _run_device(x, seg, out_len + 11)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_retimed_gpu_equals_host(monkeypatch, sample_type):
    from sushi_amd.wav import WavStream
    pcm = synth.make_dst_pcm(30, RATE, seed=21)
    w = WavStream.from_samples(pcm, RATE, sample_type=sample_type)
    on_gpu = {s: w.retimed(s) for s in (1, Fraction(25, 24), Fraction(960, 1001))}
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    for s, g in on_gpu.items():
        h = w.retimed(s)
        assert h._dev_row is None and g._dev_row is not None and g._dev_row.is_cuda
        assert g.data.dtype == h.data.dtype and g.data.shape == h.data.shape and g.data.tobytes() == h.data.tobytes()
        assert (g.sample_count, g.padding_size, g.sample_rate) == (h.sample_count, h.padding_size, h.sample_rate)
        assert g._dev_row.cpu().numpy().tobytes() == h.data.tobytes()
        assert g.device_stream().raw.cpu().numpy().tobytes() == h.data.tobytes()       # the row the searches read
    assert on_gpu[1].data.tobytes() == w.data.tobytes()


# ---------------------------------------------------------------------------------------------- a source at another speed
def _source_pcm(dst_pcm, speed):
    """The destination read at 5 s + k * speed by the same linear rule, plus white noise at 20 dB (seed 1)."""
    s = Fraction(speed)
    n = dst_pcm.shape[0]
    first = int(OFFSET_S * RATE)
    n_src = ((n - 2 - first) * s.denominator) // s.numerator + 1            # j + 1 stays inside
    t = first * s.denominator + np.arange(n_src, dtype=np.int64) * s.numerator
    j, r = t // s.denominator, t % s.denominator
    x = dst_pcm.astype(np.float64)
    y = x[j] + (r.astype(np.float64) / s.denominator) * (x[j + 1] - x[j])
    sigma = math.sqrt(float(np.mean(x ** 2)) / 10.0 ** (20.0 / 10.0))
    y = y + np.random.default_rng(1).standard_normal(n_src) * sigma
    return np.clip(np.round(y), -32768, 32767).astype(np.int16)


@pytest.fixture(scope="module")
def job():
    """dst = make_dst_pcm(150, 12000, seed=3) as a uint8 stream, and sources at other speeds made from it on demand."""
    from sushi_amd.wav import WavStream
    dst_pcm = synth.make_dst_pcm(150, RATE, seed=3)
    cache = {"dst": WavStream.from_samples(dst_pcm, RATE, sample_type="uint8")}

    def source(speed):
        speed = Fraction(speed)
        if speed not in cache:
            cache[speed] = WavStream.from_samples(_source_pcm(dst_pcm, speed), RATE, sample_type="uint8")
        return cache[speed]
    return cache["dst"], source


@pytest.mark.parametrize("speed", [Fraction(1), Fraction(25, 24), Fraction(1001, 1000), Fraction(960, 1001)])
def test_estimate_speed_names_the_true_speed(job, speed):
    dst, source = job
    est = retime.estimate_speed(source(speed), dst, probes=4)
    print("true %s: speed %s best %s fitted %r offset %r scores %s seconds %.3f" % (
        speed, est.speed, est.best, est.fitted, est.offset_seconds, np.array2string(est.scores, precision=4), est.seconds))
    assert est.probe_scores.shape == (len(retime.STANDARD_SPEEDS), 4)
    assert est.speed == speed
    assert est.scores[list(est.candidates).index(speed)] < 0.05
    assert abs(est.fitted - float(speed)) <= 1e-5
    assert abs(est.offset_seconds - OFFSET_S) <= 2.0 / RATE


def test_patterns_of_the_retimed_source_are_found_where_they_lie(job, oracle):
    dst, source = job
    speed = Fraction(25, 24)
    src = source(speed).retimed(speed)
    rng = np.random.default_rng(31)
    last = source(speed).duration_seconds - 6.0
    starts = np.linspace(4.0, last, 12) + rng.uniform(0.0, 1.0, 12)
    lengths = rng.uniform(1.0, 4.0, 12)
    f = float(speed)
    patterns = [src.get_substream(s * f, (s + l) * f) for s, l in zip(starts, lengths)]
    truth = [OFFSET_S + s * f for s in starts]
    centres = [t + (3.0 if k % 2 else -3.0) for k, t in enumerate(truth)]
    scores, times = dst.find_substreams(patterns, centres, [10.0] * 12)
    odst = oracle.OracleWavStream(dst.data, dst.sample_rate, dst.sample_count, dst.padding_size)
    for p, c, s, t, want in zip(patterns, centres, scores, times, truth):
        rs, rt = odst.find_substream(p, c, 10.0)
        print("event at %.4f: found %.6f oracle %.6f score %.6f oracle %.6f" % (want, t, rt, float(s), float(rs)))
        assert t == rt
        assert abs(float(s) - float(rs)) <= 1e-4 * float(rs) + 2.5e-7
        assert abs(t - want) <= 1.0 / RATE


def _groups(n, duration, seed):
    from sushi_amd.shifts import ScriptEvent
    events = synth.make_events(n, duration, 5, seed=seed, min_len=1.0, max_len=4.0)
    return [[ScriptEvent(s, e)] for s, e in events]


def test_shifts_at_speed_one_are_the_plain_function_s(job):
    from sushi_amd.shifts import calculate_shifts_at_speed, calculate_shifts_batched
    dst, source = job
    src = source(1)
    plain, shadowed = _groups(20, 140, 41), _groups(20, 140, 41)
    calculate_shifts_batched(src, dst, plain, 10, 30, 5)
    calculate_shifts_at_speed(src, dst, shadowed, 1, 10, 30, 5)
    for (a,), (b,) in zip(plain, shadowed):
        assert (a.shift, a.diff, a.linked) == (b.shift, b.diff, b.linked)
        assert abs(a.shift - OFFSET_S) <= 1.0 / RATE


@pytest.mark.parametrize("batched", [True, False])
def test_shifts_at_speed_carry_events_to_the_destination_s_clock(job, batched):
    from sushi_amd.shifts import calculate_shifts_at_speed
    dst, source = job
    speed = Fraction(25, 24)
    groups = _groups(20, 135, 42)
    calculate_shifts_at_speed(source(speed), dst, groups, speed, 10, 30, 5, batched=batched)
    for (e,) in groups:
        assert not e.linked
        assert abs(e.start + e.shift - (OFFSET_S + e.start * 25 / 24)) <= 1.0 / RATE, (e.start, e.shift, e.diff)
