"""The streams of the loudness-contour scenarios (tests/test_envelope_host.py, tests/test_envelope_gpu.py): one programme, 150 s
at 12 kHz, as a destination and as sources whose waveforms differ from it while the contour is the same.

The contour is |a 2000-sample moving average of N(0, 1)| (syllable-like, about 6 Hz), normalised to mean 1, squared, times a slow
scene level 0.3 + |sin(2 pi t / 7.3 s)|; a carrier is an 8-sample moving average of N(0, 1).  The destination is contour x carrier
1; every source is 3.7 s ahead of it (source instant t is destination instant t + 3.7 s):
  same           the shifted destination plus noise of 0.05 sigma (two encodes of one master: the control)
  inverted       the negative of `same`
  other_carrier  the shifted contour x carrier 2
  speed          the contour read at 25/24 (np.interp) x a carrier 2 of its own length: faster, pitch kept; no 3.7 s offset
"""
import functools
from fractions import Fraction

import numpy as np

from sushi_amd import synth

RATE, SECONDS, OFFSET_SECONDS, WINDOW = 12000, 150, 3.7, 20.0
N = SECONDS * RATE
OFFSET = int(OFFSET_SECONDS * RATE)            # 44400 samples: a multiple of hop 8
HOP, SPAN = 8, 4
SPEED = Fraction(25, 24)
CASES = ("same", "inverted", "other_carrier")


def _lp(x, k):
    c = np.cumsum(np.concatenate([[0.0], x]))
    return (c[k:] - c[:-k]) / k


def _carrier(seed, n=N):
    return _lp(np.random.default_rng(seed).standard_normal(n + 7), 8)


def to_pcm(x):
    return np.clip(x / np.abs(x).max() * 16000, -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def signals():
    """{name: float64 samples} of the destination ('dst'), the three shifted sources and the sped-up one ('speed')."""
    rng = np.random.default_rng(5)
    contour = np.abs(_lp(rng.standard_normal(N + 1999), 2000))
    contour = contour / contour.mean()
    scene = 0.3 + np.abs(np.sin(np.arange(N) * 2 * np.pi / (7.3 * RATE)))
    e = contour ** 2 * scene
    dst = e * _carrier(1)
    shifted = lambda x: np.concatenate([x[OFFSET:], np.zeros(OFFSET)])
    same = shifted(dst) + 0.05 * dst.std() * rng.standard_normal(N)
    ns = int(N / SPEED)
    e_fast = np.interp(np.arange(ns) * float(SPEED), np.arange(N), e)
    return {"dst": dst, "same": same, "inverted": -same, "other_carrier": shifted(e) * _carrier(2),
            "speed": e_fast * _carrier(2, ns)}


@functools.lru_cache(maxsize=None)
def stream(name, sample_type):
    """The WavStream of one signal (int16 at a peak of 16000 through the load pipeline); built once per process and path."""
    from sushi_amd.wav import WavStream
    return WavStream.from_samples(to_pcm(signals()[name]).astype(np.float32), RATE, sample_type=sample_type)


def events(speed=1):
    """24 events of 2-4 s; for the sped-up source they lie on its own, shorter clock."""
    return synth.make_events(24, SECONDS / float(speed), 4.0, seed=3, min_len=2.0, max_len=4.0)


def requests(src, dst, evs, scale=1.0):
    """(patterns, centres, first sample of every pattern in src's body) of a search of `evs` (seconds in src, times `scale`: the
    clock of a retimed source) in dst around each event's own time."""
    spans = [(s * scale, e * scale) for s, e in evs]
    pats = [src.get_substream(s, e) for s, e in spans]
    starts = np.array([src._get_sample_for_time(s) - src.padding_size for s, _e in spans], np.int64)
    return pats, [s for s, _e in spans], starts


def found_shifts(dst, pats, centres, starts, search):
    """The shift (samples of dst's rate) each pattern is found at: search(window row, pattern) -> arg-max index, over
    find_substream's window of +-WINDOW seconds."""
    out = []
    for p, c, s0 in zip(pats, centres, starts):
        _st, lo, n_pos = dst._window(p.shape[1], c, WINDOW)
        k = search(dst.data[:, lo:lo + n_pos + p.shape[1] - 1], p)
        out.append(lo + int(k) - dst.padding_size - int(s0))
    return np.array(out, np.int64)


# ---- rows for the bitwise comparisons
def samples(n, dtype, seed=0):
    """uint8: every value; float32: mixed magnitudes about the centre, 2^-20 .. 2^4 away from it, on either side."""
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, n, dtype=np.uint8)
    return (0.5 + rng.choice([-1.0, 1.0], n) * rng.random(n) * 2.0 ** rng.integers(-20, 5, n)).astype(np.float32)


def order_case():
    """Four float32 samples whose deviations, summed one after the other, land exactly on a float32 tie, and summed in pairs land
    above it: d = 2^31 + 0.5, 127.5, and twice 3 * 2^-24 (0.375 of the float64 spacing at 2^31).  One after the other each small
    term rounds away: E = 2^31 + 128, E / 2 = 2^30 + 64 ties to even, 2^30.  In pairs the small terms make 0.75 of the spacing
    first and round up: the result is 2^30 + 128."""
    return np.array([-2.0 ** 31, 128.0, 0.5 + 3 * 2.0 ** -24, 0.5 + 3 * 2.0 ** -24], np.float32)
