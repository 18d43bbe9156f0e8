"""What tests/test_track_wide_host.py and tests/test_track_wide_gpu.py share: rows with planted ties for the wide window minimum,
and synthetic sequences whose reaches pass 1024."""
import numpy as np

NS = (1, 2, 1025, 1026, 1027, 2051, 2052, 2053, 3079, 4104, 5000)          # below, at and above one and several window tiles of 1024
REACHES = (1025, 1500, 2047, 2048, 2049, 4999, 32767)                        # below, equal to and above n - 1 and the tile sizes
MIXED_REACH = [0, 7, 1025, 64, 3000]
# (rows, shifts, reach): 1025 on axes of one tile and two values, of two and of four tiles and a bit; a reach wider than the axis;
# the widest reach on an axis just above it and on a long one
SHAPES = [(4, 1026, 1025), (4, 2053, 1025), (4, 4104, 1025), (4, 1000, 1500), (4, 32769, 32767), (4, 70001, 32767)]
KINDS = ("random", "few_values", "both_sides", "one_side", "own", "runs", "zeros", "constant")


def tie_row(n, kind, seed=0, at=None):
    """A float64 row of n values (every one a float32 value, >= 0) with the ties `kind` names, around index `at` (default n // 2):
    random       no planted tie (float32 randoms);
    few_values   values 0, 1/4, 1/2, 3/4 only: ties everywhere;
    both_sides   the minimum at at - a and at + a, for a = 1, 300 and 1100 by turns along the axis (the negative move wins);
    one_side     several equal minima inside one side (the nearest wins);
    own          an own value equal to the window's minimum on both sides (no move);
    runs         runs of one value across the tile boundary at 1024, around `at` and at both ends of the axis;
    zeros        0.0 and -0.0 mixed at the minimum: at d = 0 and at d != 0;
    constant     one value."""
    rng = np.random.default_rng(seed * 7919 + n)
    at = n // 2 if at is None else at
    x = (rng.random(n, dtype=np.float32) * np.float32(0.25) + np.float32(0.5)).astype(np.float64)
    put = lambda where, v: x.__setitem__([k for k in where if 0 <= k < n], v)
    if kind == "few_values":
        x = rng.integers(0, 4, n).astype(np.float64) / 4.0
    elif kind == "both_sides":
        for k, a in enumerate((1, 300, 1100, 1, 300, 1100)):
            c = at + (k - 3) * 2300
            put([c - a, c + a], 0.25)
    elif kind == "one_side":
        put([at + 5, at + 9, at + 700, at + 1023, at + 1024, at + 1025, at - 2000, at - 2001], 0.25)
    elif kind == "own":
        put([at - 1030, at, at + 1030, 0, n - 1], 0.25)
    elif kind == "runs":
        put(range(1019, 1031), 0.375)
        put(range(at - 2, at + 3), 0.375)
        put(range(0, 3), 0.375)
        put(range(n - 3, n), 0.375)
    elif kind == "zeros":
        put([at - 1500, at - 3, at, at + 1, at + 1200, 0, n - 1], 0.0)
        put([at - 1499, at - 4, at + 2, at + 1201, 1, n - 2], -0.0)
    elif kind == "constant":
        x[:] = 0.625
    return x


def sequence(E, n, method, seed=0, kinds=None, at=None):
    """(curves, rows, weights): E float32 rows of n shifts at odd offsets of one buffer, weights 1, 1/2, 1 and 2 by turns (dyadic:
    with values that are multiples of 2^-24 below 1 the sums stay exact for a few rows, so planted ties stay ties), row e a
    tie_row of kinds[e % len(kinds)] -- negated for 'ccoeff_normed', so that its costs are the row's."""
    kinds = KINDS if kinds is None else kinds
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    stride = n + 3 + ((n + 3) & 1)                   # even: every row starts at an odd offset
    curves = np.zeros(E * stride + 8, np.float32)
    rows, weights = [], []
    for e in range(E):
        off = 1 + e * stride + 2 * (e % 2)
        curves[off:off + n] = tie_row(n, kinds[e % len(kinds)], seed=seed + e, at=at).astype(np.float32) * sign
        weights.append((1.0, 0.5, 1.0, 2.0)[e % 4])
        rows.append((off, weights[-1]))
    return curves, rows, weights


def rows_of(curves, rows, n):
    return [curves[o:o + n] for o, _w in rows]


# ---------------------------------------------------------------------------------------------- the long-gap scenario
# tests/track_cases.py's ten events in uint8 streams at 12 kHz, but with 20 s more without an event in front of event 5 (36 s
# streams), and no cut: the shift wanders by some tens of samples from event to event and drifts by 1890 samples across the long
# stretch -- an analogue source, two unlocked captures.  It changes at the midpoint of each gap between events.  At GAP_MAX_RATE the
# reach into event 5 is 2399 samples: a plain call refuses it; clipped to 1024 the pass cannot walk the 1890 samples and pays a
# jump.  GAP_DECOY: the destination segment of event 5 is copied GAP_DECOY samples off its true place -- 610 samples from event 4's
# shift, inside a clipped reach -- and white noise of standard deviation GAP_NOISE (int16 units) is added at the true place, so
# that the clean copy scores better.  The clipped pass then walks to the decoy for nothing and pays its jump one event later; the
# wide pass walks to the true place for nothing and pays no jump at all.
GAP_RATE, GAP_SECONDS, GAP_WINDOW = 12000, 36, 1.0
GAP_EVENTS = [(1.0, 1.8), (2.2, 2.9), (3.5, 4.0), (4.6, 5.5), (6.0, 6.9),
              (28.2, 28.4), (29.4, 30.1), (30.6, 31.1), (31.8, 32.6), (33.0, 33.9)]
GAP_TRUE_K = [3000, 3040, 3075, 3050, 2990, 1100, 1055, 1090, 1150, 1200]
GAP_K_LO, GAP_N_SHIFT = -12000, 24001
GAP_MAX_RATE, GAP_SLACK = 9e-3, 1
GAP_REACH = [0, 131, 142, 120, 153, 2399, 131, 131, 131, 131]     # ceil(GAP_MAX_RATE * samples between the events' starts) + 1
GAP_CLIPPED = [min(r, 1024) for r in GAP_REACH]
GAP_DECOY, GAP_NOISE, GAP_SEED = 2500, 2000.0, 35                  # the decoy of event 5 (2400 samples long) lies at shift 3600
# The penalties tried: 0.02, 0.05, 0.1, 0.25, 0.5, 1.0 and 2.0.  Without the decoy the clipped pass returns the true shifts at all
# seven and enters event 5 by a jump at all seven; the wide pass returns them without a jump at all seven.  With the decoy the clipped
# pass lands on it at all seven; the wide pass returns the true shifts from 0.25 on.  At 0.02, 0.05 and 0.1 it takes the decoy too:
# the noise at the true place costs 0.164 of score (0.1729 against 0.0086), more than the jump back -- no reach changes that.
GAP_PENALTIES, GAP_PENALTIES_BELOW_THE_NOISE = (0.25, 0.5, 1.0, 2.0), (0.02, 0.05, 0.1)
GAP_DECOY_K = GAP_TRUE_K[:5] + [GAP_TRUE_K[5] + GAP_DECOY] + GAP_TRUE_K[6:]       # where the clipped pass ends up


def gap_streams(decoy=False, sample_type='uint8'):
    """(destination, source) WavStreams of the long-gap scenario; decoy: with event 5's decoy planted."""
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    dst_pcm = synth.make_dst_pcm(GAP_SECONDS, GAP_RATE, seed=GAP_SEED).copy()
    cuts = [0] + [int(round((GAP_EVENTS[i][1] + GAP_EVENTS[i + 1][0]) / 2.0 * GAP_RATE)) for i in range(len(GAP_EVENTS) - 1)]
    src_pcm = synth.make_src_pcm(dst_pcm, list(zip(cuts, GAP_TRUE_K)), seed=GAP_SEED + 1)
    if decoy:
        rng = np.random.default_rng(GAP_SEED + 2)
        s, e = GAP_EVENTS[5]
        a, b = int(s * GAP_RATE) + GAP_TRUE_K[5], int(e * GAP_RATE) + GAP_TRUE_K[5]
        dst_pcm[a + GAP_DECOY:b + GAP_DECOY] = dst_pcm[a:b]
        noisy = dst_pcm[a:b].astype(np.float64) + rng.standard_normal(b - a) * GAP_NOISE
        dst_pcm[a:b] = np.clip(np.round(noisy), -32768, 32767).astype(np.int16)
    return tuple(WavStream.from_samples(pcm, GAP_RATE, sample_type=sample_type) for pcm in (dst_pcm, src_pcm))


def gap_scenario(dst, src):
    """(patterns, centres, bases) of the long-gap scenario's events."""
    patterns = [src.get_substream(s, e) for s, e in GAP_EVENTS]
    centres = [s for s, _e in GAP_EVENTS]
    return patterns, centres, [dst._get_sample_for_time(c) for c in centres]
