"""What tests/test_segments_host.py and tests/test_segments_gpu.py share: the two-cut scenario and its recorded oracle results, and
the synthetic sequences of the pass tests."""
import numpy as np

from sushi_amd import synth
from sushi_amd.wav import WavStream

# ---------------------------------------------------------------------------------------------- the two-cut scenario
# Ten events of 0.5 - 0.9 s (source times) in uint8 streams of 16 s at 12 kHz.  The source is the destination advanced by 3000
# samples up to source sample CUT and by -2400 samples from there on: a programme whose second half is another cut.  The
# destination segments of the events VICTIMS are copied to decoys DECOYS samples off their true places, inside the +-1 s window,
# and white noise of standard deviation NOISE (int16 units) is added at the true places: a lone search of a victim prefers the clean
# copy.  One joint search over all ten lands on the second half's shift and misplaces the first half.  The results below are the
# oracle's (oracle.match_template rows, path_host with equal weights).
RATE = 12000
SECONDS = 16
EVENTS = [(1.0, 1.8), (2.2, 2.9), (3.5, 4.0), (4.6, 5.5), (6.0, 6.9), (8.2, 9.0), (9.4, 10.1), (10.6, 11.1), (11.8, 12.6), (13.0, 13.9)]
CUT = 90000
OFFSETS = [(0, 3000), (CUT, -2400)]
VICTIMS, DECOYS = (2, 7), (-7200, 6000)
SEED, NOISE = 21, 2000.0
WINDOW = 1.0
PENALTY = 0.5
K_LO, N_SHIFT = -12000, 24001                       # joint_window of the scenario
TRUE_K = [3000] * 5 + [-2400] * 5
LONE_K = [3000, 3000, -4200, 3000, 3000, -2400, -2400, 3600, -2400, -2400]      # both victims at their decoys
JOINT_K = -2400                                     # one joint search over all ten (equal weights)
COST = 2.134293772280216                            # path_host, equal weights, PENALTY
PENALTIES_THAT_FIND_THE_CUT = (0.1, 0.25, 0.5, 1.0, 2.0)
# recorded from the oracle's rows: every event's score at its true shift, and its own best score
EVENT_SCORE_BITS = [0x3dedba77, 0x3e4b470e, 0x3e4fa06a, 0x3e460109, 0x3e001815, 0x3ded9dee, 0x3e2a5e1b, 0x3e670843, 0x3e2354cd,
                    0x3e061c5b]
OWN_SCORE_BITS = [0x3dedba77, 0x3e4b470e, 0x3de0e4c5, 0x3e460109, 0x3e001815, 0x3ded9dee, 0x3e2a5e1b, 0x3dfddfe2, 0x3e2354cd,
                  0x3e061c5b]
# the other penalties the oracle was asked: (penalty, shifts, cost)
EXTREMES = [(0.0, LONE_K, 1.4396894723176956),                                   # every event its lone answer
            (0.05, [3000] * 5 + [-2400, -2400, 3600, -2400, -2400], 1.6826384976506235),    # event 7 still at its decoy
            (5.0, [-2400] * 10, 3.752501204609871)]                              # one segment: a change no longer pays


def true_offset(event):
    s = EVENTS[event][0]
    return OFFSETS[1][1] if int(s * RATE) >= CUT else OFFSETS[0][1]


def two_cut_streams():
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
    return (WavStream.from_samples(dst_pcm, RATE, sample_type='uint8'), WavStream.from_samples(src_pcm, RATE, sample_type='uint8'))


def scenario(dst, src):
    """(patterns, centres, bases) of the scenario's events."""
    patterns = [src.get_substream(s, e) for s, e in EVENTS]
    centres = [s for s, _e in EVENTS]
    return patterns, centres, [dst._get_sample_for_time(c) for c in centres]


def oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift, method="sqdiff_normed"):
    """Every pattern's score row over displacements k_lo .. k_lo + n_shift - 1 from its base, by the CPU oracle."""
    return [oracle.match_template(dst.data[0, b + k_lo:b + k_lo + n_shift + p.shape[1] - 1], p[0], method=method)[0]
            for b, p in zip(bases, patterns)]


# ---------------------------------------------------------------------------------------------- synthetic sequences
SHAPES = [(1, 1), (2, 63), (7, 64), (9, 65), (33, 1023), (3, 4097), (16, 70001)]      # (rows, shifts): one sequence each
PER_LARGE_FROM = 1023 * 2048 + 1                    # the shifts from which on a workgroup takes eight indices per thread


def sequence(E, n, method, seed=0, plant=True):
    """One synthetic sequence: (curves, rows, weights, penalty) -- a curve buffer in which the E rows of n shifts lie in shuffled
    order at odd offsets, the (curve_off, weight) rows in event order.  Values are float32 in [0.25, 0.75) ('sqdiff_normed') or
    [-0.5, 0) ('ccoeff_normed'); weights 1, 1/3, 0 and 2.5 by turns (E > 2), else 1.  Every row holds a dip to the better side at a
    position that moves after every third row (so that paths stay and jump).  plant: in the (33, 1023) sequence every row's best
    value twice, at 511 and 512 (a minimum tie across a workgroup boundary); in the (3, 4097) sequence at 4095 and 4096 (a tie in
    the last element); the (9, 65) sequence is all ones."""
    rng = np.random.default_rng(seed * 1000003 + E * 131 + n)
    order = rng.permutation(E)
    offs = np.zeros(E, np.int64)
    at = 1
    for r in order:
        offs[r] = at
        at += n + 1 + 2 * int(rng.integers(0, 3))
        at += (at + 1) % 2                                             # keep every offset odd
    lo = 0.25 if method == "sqdiff_normed" else -0.5
    curves = rng.random(at, dtype=np.float32) * np.float32(0.5) + np.float32(lo)
    good = np.float32(0.1875 if method == "sqdiff_normed" else 0.125)   # a dip: better than every random value
    best = np.float32(0.125 if method == "sqdiff_normed" else 0.875)    # better than the dip
    kinds = [1.0, 1.0 / 3.0, 0.0, 2.5]
    weights = [kinds[i % 4] if E > 2 else 1.0 for i in range(E)]
    for e in range(E):
        curves[offs[e] + (7 + 37 * (e // 3)) % n] = good
        if plant and (E, n) == (9, 65):
            curves[offs[e]:offs[e] + n] = 1.0
        if plant and (E, n) == (33, 1023):
            curves[offs[e] + 511] = curves[offs[e] + 512] = best
        if plant and (E, n) == (3, 4097):
            curves[offs[e] + 4095] = curves[offs[e] + 4096] = best
    return curves, [(int(offs[e]), weights[e]) for e in range(E)], weights, 0.0625


def rows_of(curves, rows, n):
    return [curves[o:o + n] for o, _w in rows]


def stay_words(rows, weights, lam, method):
    """The stay bits of a sequence, from the definition in NumPy: [E][ceil(n / 64)] uint64, row 0 and tail bits zero."""
    E, n = len(rows), rows[0].shape[0]
    words = (n + 63) // 64
    out = np.zeros((E, words), np.uint64)
    D = None
    for e in range(E):
        c = rows[e].astype(np.float64)
        u = weights[e] * (-c if method == "ccoeff_normed" else c)
        if e == 0:
            D = u
            continue
        jump = D[int(np.argmin(D))] + lam
        stay = D <= jump
        D = u + np.where(stay, D, jump)
        bits = np.zeros(words * 64, np.uint64)
        bits[:n] = stay
        out[e] = (bits.reshape(words, 64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return out
