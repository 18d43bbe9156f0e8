"""The cases of the levelling tests (tests/test_level_host.py, tests/test_level_gpu.py): hand cases with their expected samples as
literals, a case that pins the order of the float32 window sum, the grid of the bitwise comparisons, and the dub scenario.

The dub scenario: two mono dubs of a 60 s programme.  Both carry the same music-and-effects bed (synth.make_dst_pcm(60, seed 0)),
the source 1234 samples ahead of the destination; each carries speech of its own on top, 14 dB above the bed and gated into
syllables of 0.12 .. 0.35 s with pauses of 0.05 .. 0.25 s.  A normalised score weights each instant by its energy, so the loud,
unrelated speech decides the plain search; levelled() on both streams lets the bed in the pauses count as much as the words.
"""
import functools
import math

import numpy as np

from sushi_amd import synth

RATE, SECONDS, OFFSET, WINDOW = 12000, 60, 1234, 2.0
SPEECH_DB = 14.0
SPEECH_SEEDS = {"dst": 12, "src": 13}
PEAK_AT = 30000.0


# ---------------------------------------------------------------------------------------------- the dub scenario
def gate(seed, n):
    """n samples of a syllable gate: on for int(U(0.12, 0.35) * RATE) samples, off for int(U(0.05, 0.25) * RATE), alternately and
    starting on, smoothed with a Hann window of 121 samples of sum 1."""
    rng = np.random.default_rng(seed)
    g = np.zeros(n, np.float64)
    pos, on = 0, True
    while pos < n:
        length = int(rng.uniform(0.12, 0.35) * RATE) if on else int(rng.uniform(0.05, 0.25) * RATE)
        if on:
            g[pos:pos + length] = 1.0
        pos += length
        on = not on
    win = np.hanning(121)
    return np.convolve(g, win / win.sum(), mode="same")


@functools.lru_cache(maxsize=None)
def signals():
    """{'dst', 'src'}: float64 samples, the larger peak of the two at PEAK_AT."""
    bed = synth.make_dst_pcm(SECONDS, RATE, seed=0).astype(np.float64)
    n = bed.shape[0]
    bed_rms = math.sqrt(float(np.mean(bed ** 2)))
    beds = {"dst": bed, "src": np.concatenate([bed[OFFSET:], np.zeros(OFFSET)])}
    out = {}
    for name, s in SPEECH_SEEDS.items():
        speech = synth.make_dst_pcm(SECONDS, RATE, seed=s).astype(np.float64)
        speech = speech / math.sqrt(float(np.mean(speech ** 2)))
        out[name] = beds[name] + speech * gate(s + 100, n) * bed_rms * 10.0 ** (SPEECH_DB / 20.0)
    scale = PEAK_AT / max(float(np.abs(v).max()) for v in out.values())
    return {name: v * scale for name, v in out.items()}


def stream(name, sample_type):
    """The WavStream of one signal through the load pipeline (on whichever path the process is on)."""
    from sushi_amd.wav import WavStream
    return WavStream.from_samples(signals()[name].astype(np.float32), RATE, sample_type=sample_type)


def events():
    return synth.make_events(24, float(SECONDS), WINDOW, seed=5, min_len=1, max_len=3)


# ---------------------------------------------------------------------------------------------- hand cases
def hand_cases():
    """(samples, in_start, window, floor, peak, expected samples), every output worked out by hand.  With floor = 1 / 128, fw is
    W steps of a uint8 stream (W) and W / 256 on float32; the float32 samples are 0.5 + k / 256, the same deviations k in units
    of 1 / 256, so that every quotient is the same fraction on both sample types."""
    fl = 1.0 / 128
    f = lambda ks: np.array([0.5 + k / 256.0 for k in ks], np.float32)
    u = lambda ks: np.array([128 + k for k in ks], np.uint8)
    return [
        # W = 1, peak 1: E = |d|, q = d / (|d| + 1): 127/128, -128/129, 0, 1/2, -1/2, 3/4, 7/8 -> floor(q * 128 + 128.5):
        # 255.5, 1.49.., 128.5, 192.5, 64.5, 224.5, 240.5
        (u([127, -128, 0, 1, -1, 3, 7]), 0, 1, fl, 1.0, [255, 1, 128, 192, 64, 224, 240]),
        # ... and on float32: 0.5 + q / 2 for q = 0, 1/2, -1/2, 3/4, 7/8, -3/4
        (f([0, 1, -1, 3, 7, -3]), 0, 1, fl, 1.0, [0.5, 0.75, 0.25, 0.875, 0.9375, 0.125]),
        # W = 3 over a row of three, d = 1, -3, 9: both clamps of the row act.  E = 1 + 1 + 3, 1 + 3 + 9, 3 + 9 + 9 and fw = 3:
        # q = 3 / 8, -9 / 16, 27 / 24 -> 1.  uint8: 48 + 128.5, -72 + 128.5 = 56.5, 256.5 -> 255
        (u([1, -3, 9]), 0, 3, fl, 1.0, [176, 56, 255]),
        (f([1, -3, 9]), 0, 3, fl, 1.0, [0.6875, 0.21875, 1.0]),
        # the same from in_start = n_in - 1: the last sample again, and one past the row: d = 9, E = 27, q = 27 / 30 = 0.9 ->
        # floor(115.2 + 128.5) = 243
        (u([1, -3, 9]), 2, 3, fl, 1.0, [255, 243]),
        (f([1, -3, 9]), 2, 3, fl, 1.0, [1.0, 0.949999988079071]),          # float32(0.5 + 0.5 * 0.9)
        # q held on either side by a small peak, W = 1: d = 127, -128, 1, -1, 0 at peak 1/2: q = 127 / 64, -128 / 64.5, 1, -1, 0;
        # q = 1 gives floor(256.5) = 256, held to 255; q = -1 gives floor(0.5) = 0
        (u([127, -128, 1, -1, 0]), 0, 1, fl, 0.5, [255, 0, 255, 0, 128]),
        # float32 at peak 1/4: d = +-1/256: q = +-2 -> +-1; d = 3/256: q = 3 -> 1; d = 0
        (f([1, -1, 3, 0]), 0, 1, fl, 0.25, [1.0, 0.0, 1.0, 0.5]),
        # digital silence gives the centre, whatever the window: 0 / (fw * peak)
        (u([0] * 5), 0, 3, fl, 8.0, [128] * 5),
        (f([0] * 5), 2, 1023, fl, 8.0, [0.5] * 3),
        (u([0] * 2), 1, 129, 2.0 ** -20, 0.75, [128] * 4),
        # the uint8 roundings at a half, W = 1, peak 128: q * 128 = d / (|d| + 1): 1/2 -> floor(129.0) = 129 (up), -1/2 ->
        # floor(128.0) = 128 (up), 3/4 -> 129, -3/4 -> floor(127.75) = 127, 127/128 -> 129
        (u([1, -1, 3, -3, 127]), 0, 1, fl, 128.0, [129, 128, 129, 127, 129]),
        # W = 3 inside a constant row d = 6 at peak 32: E = 18, fw = 3, q * 128 = 18 * 128 / (21 * 32) = 24 / 7 -> floor(131.9..)
        (u([6] * 4), 1, 3, fl, 32.0, [131, 131]),
    ]


# ---------------------------------------------------------------------------------------------- the order of the float32 sum
# W = 9 at in_start 4 of nine samples: |d| = 2^30 - 0.5, then eight of 2^-24 (half a unit in the last place of the first: added
# one by one after it, each is lost to the tie's even neighbour; added up first, they are four units).  The centre sample lies
# below 0.5, and peak puts q within 2^-29 of -1: there 0.5 + 0.5 * q is exact and near 2^-30, where float32's spacing is 2^-53,
# so a window sum four units off moves the output by a float32 step.
ORDER_SAMPLES = [2.0 ** 30] + [0.5 + 2.0 ** -24] * 3 + [0.5 - 2.0 ** -24] + [0.5 + 2.0 ** -24] * 4      # float32 holds each exactly
ORDER_WINDOW, ORDER_FLOOR, ORDER_PEAK = 9, 2.0 ** -20, float.fromhex("0x1.2000000b3ffedp-51")
ORDER_SEQUENTIAL = 9.31322685637781e-10       # t = 0 .. 8: sushi_hip_level's
ORDER_REVERSED = 9.313227966600834e-10        # t = 8 .. 0
ORDER_PAIRWISE = 9.313227966600834e-10        # ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + (a7 + a8)))


def order_case():
    """(samples, in_start, window, floor, peak): one output whose float32 value tells the sequential window sum from the reversed
    and the pairwise one."""
    return np.array(ORDER_SAMPLES, np.float32), 4, ORDER_WINDOW, ORDER_FLOOR, ORDER_PEAK


# ---------------------------------------------------------------------------------------------- the bitwise comparisons
WINDOWS = (1, 3, 129, 1023)
ROWS = (1, 2, 300, 70001)                     # filter_cases.samples: every byte value, float32 magnitudes 2^-20 .. 2^4
OUT_LENS = (1, 2, 257, 2049, 40000)
PAIRS = [(fl, pk) for fl in (1.0 / 128, 2.0 ** -20) for pk in (8.0, 1.0, 0.75)]        # (floor, peak)


def starts(n_in):
    return sorted({0, min(5, n_in - 1), n_in - 1})


def launch_shape(dtype, window):
    """(outputs a tile, the most workgroups of a launch, LDS bytes) as level_core.hpp states them.  float32: 256 threads with 8
    outputs each, element e of the tile's 2048 + W - 1 staged float64 in slot e + e // 8.  uint8: 16 outputs each; 256 * 21 + 8
    words of prefix sums and waves' totals and 256 * 21 staged bytes.  As many workgroups as 256 CUs of 160 KB hold, four a CU
    at the most."""
    if np.dtype(dtype) == np.uint8:
        tile, lds = 4096, (256 * 21 + 8) * 4 + 256 * 21
    else:
        e = 2048 + window - 2
        tile, lds = 2048, (e + e // 8 + 1) * 8
    return tile, 256 * min(4, 160 * 1024 // lds), lds
