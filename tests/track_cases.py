"""What tests/test_track_host.py and tests/test_track_gpu.py share: the wandering-shift scenario and its recorded oracle results,
and the synthetic sequences of the pass tests."""
import numpy as np

import segment_cases
from sushi_amd import synth
from sushi_amd.wav import WavStream

# ---------------------------------------------------------------------------------------------- the wandering-shift scenario
# tests/segment_cases.py's ten events in uint8 streams of 16 s at 12 kHz -- but the source's shift is another for every event: it
# wanders by some tens of samples from event to event (two hours of wander on unlocked clocks compressed into 16 s), and there is a
# cut in the middle.  The shift changes at the midpoint of each gap between events.  The destination segments of the events VICTIMS
# are copied to decoys DECOYS samples off their true places, inside the +-1 s window, and white noise of standard deviation NOISE
# (int16 units) is added at the true places: a lone search of a victim prefers the clean copy.  The segmentation pass charges one
# price for a change to the true neighbour and for a change to a decoy: it either follows the decoys or collapses to one shift.
# The results below are the oracle's (oracle.match_template rows; path_host and track_host with equal weights).
RATE, SECONDS, EVENTS, WINDOW = segment_cases.RATE, segment_cases.SECONDS, segment_cases.EVENTS, segment_cases.WINDOW
K_LO, N_SHIFT = segment_cases.K_LO, segment_cases.N_SHIFT
TRUE_K = [3000, 3040, 3075, 3050, 2990, -2400, -2445, -2410, -2350, -2300]
VICTIMS, DECOYS = (2, 7), (-7200, 6000)
SEED, NOISE = 31, 2000.0
MAX_RATE, SLACK = 6e-3, 1
REACH = [0, 88, 95, 81, 102, 160, 88, 88, 88, 88]      # ceil(MAX_RATE * samples between the events' starts) + SLACK
LONE_K = [3000, 3040, -4125, 3050, 2990, -2400, -2445, 3590, -2350, -2300]       # both victims at their decoys
PATH_PENALTIES = (0.1, 0.25, 0.5, 1.0, 2.0)            # the segmentation pass is wrong at every one of them
TRACK_PENALTIES, STEP_COSTS = (0.1, 0.25, 0.5, 1.0), (0.0, 1e-3)     # the tracking pass is right at the eight combinations
PENALTY_TOO_LARGE = 2.0                                # ... and no longer pays for the cut at this one
PENALTY = 0.5
# recorded from the oracle's rows.  path_host: (penalty, shifts, cost) -- the lone arg-mins; neighbours dragged onto the decoys; one shift
PATH_RESULTS = [(0.1, LONE_K, 2.513500662147999),
                (0.25, [3000, -4125, -4125, -4125, 2990, -2400, 3590, 3590, 3590, -2300], 3.699646480381489),
                (0.5, [3000] * 10, 4.695971444249153), (1.0, [3000] * 10, 4.695971444249153), (2.0, [3000] * 10, 4.695971444249153)]
# track_host: cost by (penalty, step_cost); the path is TRUE_K at all eight
TRACK_COSTS = {(0.1, 0.0): 1.833965739607811, (0.1, 1e-3): 2.183965739607811, (0.25, 0.0): 1.983965739607811,
               (0.25, 1e-3): 2.3339657396078106, (0.5, 0.0): 2.233965739607811, (0.5, 1e-3): 2.583965739607811,
               (1.0, 0.0): 2.733965739607811, (1.0, 1e-3): 3.083965739607811}
TOO_LARGE_K = [3000, 3040, 3075, 3050, 2990, 2965, 2985, 3026, 3097, 3107]      # PENALTY_TOO_LARGE, step_cost 0: the cut is walked
# every event's score at its true shift, and its own best score
EVENT_SCORE_BITS = [0x3e087031, 0x3e6433a5, 0x3e333096, 0x3e635890, 0x3e0dd1b8, 0x3e00d418, 0x3e40786e, 0x3e53d9e8, 0x3e36f3ad,
                    0x3e127be8]
OWN_SCORE_BITS = [0x3e087031, 0x3e6433a5, 0x3def7f27, 0x3e635890, 0x3e0dd1b8, 0x3e00d418, 0x3e40786e, 0x3e13efb8, 0x3e36f3ad,
                  0x3e127be8]
JUMPS = [5]                                            # the cut: the one event entered by a jump


def pieces():
    """[(first source sample, shift)]: event i's shift from the midpoint of the gap in front of it on."""
    cuts = [0] + [int(round((EVENTS[i][1] + EVENTS[i + 1][0]) / 2.0 * RATE)) for i in range(len(EVENTS) - 1)]
    return list(zip(cuts, TRUE_K))


def streams():
    """(destination, source) WavStreams of the scenario."""
    dst_pcm = synth.make_dst_pcm(SECONDS, RATE, seed=SEED).copy()
    src_pcm = synth.make_src_pcm(dst_pcm, pieces(), seed=SEED + 1)
    rng = np.random.default_rng(SEED + 2)
    for victim, decoy in zip(VICTIMS, DECOYS):
        s, e = EVENTS[victim]
        a, b = int(s * RATE) + TRUE_K[victim], int(e * RATE) + TRUE_K[victim]
        dst_pcm[a + decoy:b + decoy] = dst_pcm[a:b]
        noisy = dst_pcm[a:b].astype(np.float64) + rng.standard_normal(b - a) * NOISE
        dst_pcm[a:b] = np.clip(np.round(noisy), -32768, 32767).astype(np.int16)
    return (WavStream.from_samples(dst_pcm, RATE, sample_type='uint8'), WavStream.from_samples(src_pcm, RATE, sample_type='uint8'))


scenario, oracle_rows = segment_cases.scenario, segment_cases.oracle_rows

# ---------------------------------------------------------------------------------------------- synthetic sequences
SHAPES = [(1, 1, 0), (2, 63, 1), (7, 64, 3), (9, 65, 64), (33, 1023, 127), (3, 4097, 1024), (16, 70001, 5)]   # (rows, shifts, reach)
PER_LARGE_FROM = 1023 * 2048 + 1                    # the shifts from which on a workgroup takes eight indices per thread
STEP_COST = 2.0 ** -12                              # a dyadic price: planted ties stay ties


def reaches(E, reach):
    """One reach per row that varies by row: from row 1 on the widest, half of it, 0 and one less than the widest by turns; row 0's is ignored
    (given as 1024 + 1: a value no other row may have)."""
    kinds = [max(reach - 1, 0), reach, reach // 2, 0]
    return [1025] + [kinds[e % 4] for e in range(1, E)]


def sequence(E, n, reach, method, seed=0):
    """segment_cases.sequence's (curves, rows, weights, penalty) -- rows at odd offsets in shuffled order, weights 1, 1/3, 0 and 2.5,
    dips that move, equal values at 511 | 512 and in the last element, the all-ones sequence -- with (reaches, step_cost), and, where
    there are at least 8 shifts and the sequence is not the all-ones one, a value better than every other in each row at a place that
    wanders: from n // 3 it walks by up to 3 shifts a row, to and fro, never further than the row's reach, and in a sequence of at least 7 rows it is half the axis away from the middle
    row on -- the best path moves, and jumps."""
    curves, rows, weights, lam = segment_cases.sequence(E, n, method, seed=seed)
    rs = reaches(E, reach)
    if n >= 8 and (E, n) != (9, 65):
        better = np.float32(0.0625 if method == "sqdiff_normed" else 0.9375)
        at = n // 3
        for e, (off, _w) in enumerate(rows):
            if e:
                at = min(max(at + (-1) ** e * min(rs[e], 1 + e % 3), 0), n - 1)
            if E >= 7 and e == E // 2:
                at = (at + n // 2) % n                  # ... and jumps once, further than any reach of these sequences
            curves[off + at] = better
    return curves, rows, weights, lam, rs, STEP_COST


rows_of = segment_cases.rows_of


def tie_rows(n, centre, method):
    """Two rows of n shifts (weights 1) whose second row meets planted ties: D_0 is 0.25 (the minimum) at centre - 1 and centre + 1
    -- cand(-1) == cand(+1) at `centre` --, at 0 and 1 and at n - 2 and n - 1 (cand(0) == cand(+-1) at both ends, with step_cost
    0), and in [0.5, 0.75) elsewhere."""
    rng = np.random.default_rng(n + centre)
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    a = rng.random(n, dtype=np.float32) * np.float32(0.25) + np.float32(0.5)
    a[[centre - 1, centre + 1, 0, 1, n - 2, n - 1]] = np.float32(0.25)
    b = rng.random(n, dtype=np.float32) * np.float32(0.25) + np.float32(0.5)
    return [a * sign, b * sign]
