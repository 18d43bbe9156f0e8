"""The cases of the filter tests (tests/test_filter_host.py, tests/test_filter_gpu.py): hand cases with their expected samples as
literals, a case that pins the order of the sum, rows and taps for the bitwise comparisons, and the hum scenario.

The hum scenario: a 60 s programme (synth.make_dst_pcm(60, seed 0)) as a destination and as a source 1234 samples ahead of it,
two analogue captures that each carry their own mains hum: 50.0 Hz at phase 0.3 in the destination, 50.03 Hz at phase 2.1 in the
source, each at HUM_LEVEL x rms x sqrt(2) of amplitude (HUM_LEVEL x the programme's rms).  The hum correlates with itself at every
period and the two hums have unrelated phase, so the plain search loses the true place; a 255-tap 150 Hz high-pass on both
streams gives it back.
"""
import functools
import math

import numpy as np

from sushi_amd import synth

RATE, SECONDS, OFFSET, WINDOW = 12000, 60, 1234, 2.0
HUM_LEVEL = 2.0
HUM = ((50.0, 0.3), (50.03, 2.1))                 # (Hz, phase) in the destination, in the source
LOW, N_TAPS = 150.0, 255
SQ = "sqdiff_normed"


@functools.lru_cache(maxsize=None)
def signals():
    """{'dst', 'src'}: float64 samples with the hum on them."""
    pcm = synth.make_dst_pcm(SECONDS, RATE, seed=0).astype(np.float64)
    n = pcm.shape[0]
    amp = HUM_LEVEL * math.sqrt(float(np.mean(pcm ** 2))) * math.sqrt(2.0)
    t = np.arange(n, dtype=np.float64) / RATE
    src = np.concatenate([pcm[OFFSET:], np.zeros(OFFSET)])
    (f_dst, p_dst), (f_src, p_src) = HUM
    return {"dst": pcm + amp * np.sin(2 * np.pi * f_dst * t + p_dst), "src": src + amp * np.sin(2 * np.pi * f_src * t + p_src)}


def stream(name, sample_type):
    """The WavStream of one signal through the load pipeline (on whichever path the process is on)."""
    from sushi_amd.wav import WavStream
    return WavStream.from_samples(signals()[name].astype(np.float32), RATE, sample_type=sample_type)


def events():
    return synth.make_events(24, float(SECONDS), WINDOW, seed=5, min_len=1, max_len=3)


def requests(src, evs):
    """(patterns, centres, first sample of every pattern in src's body) of a search of `evs` (seconds in src) around each event's
    own time."""
    pats = [src.get_substream(s, e) for s, e in evs]
    starts = np.array([src._get_sample_for_time(s) - src.padding_size for s, _e in evs], np.int64)
    return pats, [s for s, _e in evs], starts


def found_shifts(dst, pats, centres, starts, search):
    """The shift (samples) each pattern is found at: search(window row, pattern) -> index of the best score, over
    find_substream's window of +-WINDOW seconds."""
    out = []
    for p, c, s0 in zip(pats, centres, starts):
        _st, lo, n_pos = dst._window(p.shape[1], c, WINDOW)
        k = search(dst.data[:, lo:lo + n_pos + p.shape[1] - 1], p)
        out.append(lo + int(k) - dst.padding_size - int(s0))
    return np.array(out, np.int64)


# ---- hand cases: (samples, in_start, taps, expected samples), every output worked out by hand
def hand_cases():
    from sushi_amd.filter import preemphasis_taps
    f32 = np.arange(9, dtype=np.float32) / np.float32(65536.0)
    return [
        # T = 1, h = [1.0]: the identity
        (np.array([0, 1, 127, 128, 129, 254, 255], np.uint8), 0, [1.0], [0, 1, 127, 128, 129, 254, 255]),
        (f32, 0, [1.0], [k / 65536.0 for k in range(9)]),
        # pre-emphasis at mu = 1/2 on a ramp of slope 2 from the centre: d = 2 i; y = d[i] - d[i - 1] / 2 = i + 1 (i = 0 reads
        # x[0] twice: 0); the third tap, 0.0, meets x[i + 1]
        (np.array([128, 130, 132, 134, 136, 138], np.uint8), 0, preemphasis_taps(0.5), [128, 130, 131, 132, 133, 134]),
        # ... and in float32: d = i / 8; y = (i + 1) / 16 for i >= 1
        (np.array([0.5 + i / 8.0 for i in range(5)], np.float32), 0, preemphasis_taps(0.5), [0.5, 0.625, 0.6875, 0.75, 0.8125]),
        # gain 2: 255 -> 254 + 128.5 -> 382, held to 255; 0 -> -256 + 128.5 -> floor -128, held to 0; 129 -> 130; 127 -> 126
        (np.array([255, 0, 129, 127], np.uint8), 0, [0.0, 2.0, 0.0], [255, 0, 130, 126]),
        # gain 1/2, halves round up: d = 127, -128, 1, -1, 3, 0 -> acc = 63.5, -64, 0.5, -0.5, 1.5, 0 -> floor(acc + 128.5)
        (np.array([255, 0, 129, 127, 131, 128], np.uint8), 0, [0.0, 0.5, 0.0], [192, 64, 129, 128, 130, 128]),
        # both clamps of the row: h = [1, 0, 0] reads x[i - 1], h = [0, 0, 1] reads x[i + 1]; from in_start 1 three outputs
        (np.array([10, 20, 30], np.uint8), 1, [1.0, 0.0, 0.0], [10, 20, 30]),
        (np.array([10, 20, 30], np.uint8), 1, [0.0, 0.0, 1.0], [30, 30, 30]),
        (np.array([10, 20, 30], np.uint8), 0, [1.0, 0.0, 0.0], [10, 10, 20]),
    ]


# ---- the order of the sum
ORDER_SAMPLES = [3.5, -2.0 ** 31, 2.0 ** 31, 0.75, 0.5 + 3 * 2.0 ** -24]       # float32 holds each exactly
ORDER_TAPS = [0.1, 1.0, 1.0 + 2.0 ** -30, 0.75, 1.0]
# float32(acc + 0.5) of the one output at in_start 2, by the order of the sum
ORDER_SEQUENTIAL = 1.9875004291534424       # k = 0 .. 4, product and sum rounded separately: sushi_hip_filter's
ORDER_REVERSED = 1.9874999523162842         # k = 4 .. 0
ORDER_PAIRWISE = 1.9875001907348633         # (p0 + p1) + (p2 + (p3 + p4))
ORDER_FMA = 1.9875003099441528              # k = 0 .. 4, acc = fma(h, d, acc)


def order_case():
    """(samples, in_start, taps): one output whose float32 value tells the four ways of summing apart.  Products 0.3, -(2^31 +
    0.5), (2^31 - 0.5)(1 + 2^-30) and two small ones: the large products cancel to about 1, and what each order loses of the
    small ones on the way, at float64's spacing of 2^-21 near 2^31, moves the result by whole float32 steps of 2^-23."""
    return np.array(ORDER_SAMPLES, np.float32), 2, np.array(ORDER_TAPS, np.float64)


# ---- rows and taps for the bitwise comparisons
def samples(n, dtype, seed=0):
    """uint8: every value; float32: mixed magnitudes about the centre, 2^-20 .. 2^4 away from it, on either side."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    return (0.5 + rng.choice([-1.0, 1.0], n) * rng.random(n) * 2.0 ** rng.integers(-20, 5, n)).astype(np.float32)


def taps(n_taps, seed=0):
    """n_taps float64 taps of mixed sign and magnitude with a sum of magnitudes near 2: the uint8 outputs use the whole range
    and both clamps; not symmetric."""
    rng = np.random.default_rng(1000 + seed + n_taps)
    h = rng.standard_normal(n_taps) * 2.0 ** rng.integers(-12, 1, n_taps)
    return h / np.abs(h).sum() * 2.0


def launch_shape(n_taps):
    """(outputs a tile, the most workgroups of a launch) at n_taps taps, as filter_core.hpp states them: 256 threads with 8
    outputs each up to 1025 taps and 4 above; element e of a tile's tile + T - 1 staged samples in slot e + e // per; LDS of
    T + 1 + slots doubles; as many workgroups as 256 CUs of 160 KB hold, five a CU at the most."""
    per = 8 if n_taps <= 1025 else 4
    tile = 256 * per
    e = tile + n_taps - 2
    lds = (n_taps + 1 + e + e // per + 1) * 8
    return tile, 256 * min(5, 160 * 1024 // lds)


TAP_COUNTS = (1, 3, 63, 255, 2047)
ROWS = (1, 2, 300, 70001)
OUT_LENS = (1, 2, 257, 40000)


def grid(n_in):
    """(in_start, out_len) over in_start 0, 5 and n_in - 1 (both clamps act) and every out_len -- 1025 and 2049 besides, one past a
    tile of either kind."""
    return [(s, m) for s in sorted({0, min(5, n_in - 1), n_in - 1}) for m in OUT_LENS + (1025, 2049)]
