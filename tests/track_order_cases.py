"""What tests/test_track_order_host.py and tests/test_track_order_gpu.py share: the decoy scenario of the ordered pass and its
recorded oracle results, and the backs and penalties of the synthetic sequences (the sequences themselves are track_cases')."""
import numpy as np

import track_cases
from sushi_amd import synth
from sushi_amd.wav import WavStream

# ---------------------------------------------------------------------------------------------- the decoy scenario
# Ten events in uint8 streams of 14 s at 12 kHz, built as tests/segment_cases.py builds its streams.  The source is the
# destination advanced by 3000 samples up to source sample CUT and by -1800 from there on: 4800 samples removed inside the one gap
# of 6000 samples between events 4 and 5 (every other gap is 3600 or 3601).  The destination segments of the events VICTIMS are copied to
# decoys DECOYS samples off their true places, inside the +-1 s window, and white noise of standard deviation NOISE (int16 units)
# is added at the true places.  A path through a decoy takes two jumps, there and back, and one of the two lowers the shift by
# 8400: that would put an event in the destination before the end of the event in front of it, which no cut does.  With the backs
# of order_back -- at most the gap between two events -- that jump does not exist; the real cut, -4800 in a gap of 6000, does.
# Reach 0, equal weights, step_cost 0.  The results below are the oracle's (oracle.match_template rows).
RATE, SECONDS, WINDOW = 12000, 14, 1.0
EVENTS = [(1.0, 1.8), (2.1, 2.9), (3.2, 3.9), (4.2, 5.0), (5.3, 6.0), (6.5, 7.3), (7.6, 8.3), (8.6, 9.2), (9.5, 10.3), (10.6, 11.4)]
CUT = 75000
OFFSETS = [(0, 3000), (CUT, -1800)]
VICTIMS, DECOYS = (2, 7), (-8400, 8400)
SEED, NOISE = 31, 9000.0
K_LO, N_SHIFT = -12000, 24001                       # joint_window of the scenario
TRUE_K = [3000] * 5 + [-1800] * 5
BACK = [None, 3600, 3600, 3600, 3600, 6000, 3600, 3600, 3601, 3600]      # order_back of the events: the gaps (None: no limit)
# penalties at which today's pass follows a decoy and the ordered pass does not; at which both are right; at which the cut no
# longer pays for either
PENALTIES_ORDER_ONLY = (0.01, 0.02, 0.03)
PENALTIES_BOTH = (0.05, 0.1, 0.25)
PENALTY_TOO_LARGE = 0.5
PENALTY = 0.02                                      # the one the GPU's end-to-end tests use
# recorded from the oracle's rows: {penalty: (track_host's shifts, its cost, track_ordered_host's shifts, its cost)}
DECOYED_A = [3000, -11407, -5400, 3000, 3000, -1800, -1800, 6600, 10965, -1800]
DECOYED_B = [3000, -11407, -5400, 3000, 3000, -1800, -1800, 6600, -1800, -1800]
RESULTS = {0.01: (DECOYED_A, 3.768427021503448, TRUE_K, 3.9098649418354032),
           0.02: (DECOYED_B, 3.835137988328934, TRUE_K, 3.9198649418354035),
           0.03: (DECOYED_B, 3.8951379883289334, TRUE_K, 3.9298649418354032),
           0.05: (TRUE_K, 3.9498649418354033, TRUE_K, 3.9498649418354033),
           0.1: (TRUE_K, 3.9998649418354035, TRUE_K, 3.9998649418354035),
           0.25: (TRUE_K, 4.149864941835403, TRUE_K, 4.149864941835403),
           0.5: ([-1800] * 10, 4.383311301469803, [-1800] * 10, 4.383311301469803)}
LONE_K = DECOYED_A                                  # every event's lone arg-min: chance matches beat both victims and two more
EVENT_SCORE_BITS = [0x3ebd0287, 0x3ed8a9b2, 0x3ed45ba2, 0x3ed5fe35, 0x3eb3fcde, 0x3ebc26bf, 0x3ec713ed, 0x3eca8c12, 0x3ed8ae7d,
                    0x3eb242f0]       # every event's score at its true shift


def true_offset(event):
    s = EVENTS[event][0]
    return OFFSETS[1][1] if int(s * RATE) >= CUT else OFFSETS[0][1]


def streams(sample_type='uint8'):
    """(destination, source) WavStreams of the scenario."""
    dst_pcm = synth.make_dst_pcm(SECONDS, RATE, seed=SEED).copy()
    src_pcm = synth.make_src_pcm(dst_pcm, OFFSETS, seed=SEED + 1)
    rng = np.random.default_rng(SEED + 2)
    for victim, decoy in zip(VICTIMS, DECOYS):
        s, e = EVENTS[victim]
        a, b = int(s * RATE) + true_offset(victim), int(e * RATE) + true_offset(victim)
        dst_pcm[a + decoy:b + decoy] = dst_pcm[a:b]
        noisy = dst_pcm[a:b].astype(np.float64) + rng.standard_normal(b - a) * NOISE
        dst_pcm[a:b] = np.clip(np.round(noisy), -32768, 32767).astype(np.int16)
    return (WavStream.from_samples(dst_pcm, RATE, sample_type=sample_type), WavStream.from_samples(src_pcm, RATE, sample_type=sample_type))


def scenario(dst, src):
    """(patterns, centres, bases) of the scenario's events."""
    patterns = [src.get_substream(s, e) for s, e in EVENTS]
    centres = [s for s, _e in EVENTS]
    return patterns, centres, [dst._get_sample_for_time(c) for c in centres]


oracle_rows = track_cases.segment_cases.oracle_rows

# ---------------------------------------------------------------------------------------------- synthetic sequences
SHAPES = track_cases.SHAPES


def backs(E, n):
    """One back per row that varies by row: 0, 1, 255, 256, n - 1, n + 7 and no limit by turns (row 0's is ignored)."""
    kinds = [0, 1, 255, 256, n - 1, n + 7, -1]
    return [-1] + [kinds[(e - 1) % 7] for e in range(1, E)]


def penalties(E, lam):
    """One penalty per row that varies by row, dyadic multiples of the sequence's own: 1, 1/4, 0, 2 and 1/2 times it by turns (row
    0's is ignored: given as NaN, a value no other row may have)."""
    kinds = [1.0, 0.25, 0.0, 2.0, 0.5]
    return [float("nan")] + [lam * kinds[(e - 1) % 5] for e in range(1, E)]


def sequence(E, n, reach, method, seed=0):
    """track_cases.sequence with (backs, penalties) in place of its one penalty: (curves, rows, weights, penalties, reaches,
    step_cost, backs)."""
    curves, rows, weights, lam, rs, mu = track_cases.sequence(E, n, reach, method, seed=seed)
    return curves, rows, weights, penalties(E, lam), rs, mu, backs(E, n)


def prefix_tie_rows(n, at, method):
    """Two rows of n shifts (weights 1) whose first row holds its minimum, 0.25, twice: at at - 1 and at (255 | 256 and 511 | 512
    are the two sides of a wave's, a round's or a work item's boundary); everything else in [0.5, 0.75)."""
    rng = np.random.default_rng(n * 7 + at)
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    a = rng.random(n, dtype=np.float32) * np.float32(0.25) + np.float32(0.5)
    a[[at - 1, at]] = np.float32(0.25)
    b = rng.random(n, dtype=np.float32) * np.float32(0.25) + np.float32(0.5)
    return [a * sign, b * sign]
