"""What tests/test_joint_host.py and tests/test_joint_gpu.py share: the decoy scenario and its recorded oracle results, and the
ragged synthetic groups of the reduce tests."""
import numpy as np

from sushi_amd import synth
from sushi_amd.wav import WavStream

# ---------------------------------------------------------------------------------------------- the decoy scenario
# Five events of 0.5 - 0.9 s (source times) in uint8 streams of 8 s at 12 kHz; the source is the destination advanced by OFFSET
# samples.  The destination segment of event VICTIM is copied to a decoy DECOY samples off its true place, inside the +-1 s window,
# and white noise of standard deviation NOISE (int16 units) is added at the true place: the victim's lone search prefers the clean
# copy, its four neighbours know better.  SEED and NOISE were chosen on the CPU oracle so that it alone shows both facts; the
# results below are the oracle's (oracle.match_template rows, joint_host with equal weights).
RATE = 12000
EVENTS = [(1.0, 1.8), (2.2, 2.9), (3.5, 4.0), (4.6, 5.5), (6.0, 6.9)]
VICTIM, OFFSET, DECOY = 2, 3000, -7200
SEED, NOISE = 21, 2000.0
WINDOW = 1.0
K_LO, N_SHIFT = -12000, 24001                       # joint_window of the scenario
LONE_K = [3000, 3000, -4200, 3000, 3000]            # where each event's lone arg-min lies: the victim's is the decoy (OFFSET + DECOY)
JOINT_K = 3000                                      # where joint_host's lies: the true shift
JOINT_SCORE_BITS = 0x3e856f6d
VICTIM_LONE_SCORE_BITS = 0x3e21fa47
EVENT_SCORE_BITS = [0x3e2d2eb6, 0x3eaede14, 0x3e8c42e6, 0x3eaa5936, 0x3e3e372d]


def decoy_streams():
    """(destination, source) WavStreams of the scenario."""
    dst_pcm = synth.make_dst_pcm(8, RATE, seed=SEED).copy()
    src_pcm = synth.make_src_pcm(dst_pcm, OFFSET, seed=SEED + 1)
    s, e = EVENTS[VICTIM]
    a, b = int(s * RATE) + OFFSET, int(e * RATE) + OFFSET
    dst_pcm[a + DECOY:b + DECOY] = dst_pcm[a:b]
    rng = np.random.default_rng(SEED + 2)
    noisy = dst_pcm[a:b].astype(np.float64) + rng.standard_normal(b - a) * NOISE
    dst_pcm[a:b] = np.clip(np.round(noisy), -32768, 32767).astype(np.int16)
    return (WavStream.from_samples(dst_pcm, RATE, sample_type='uint8'), WavStream.from_samples(src_pcm, RATE, sample_type='uint8'))


def oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift, method="sqdiff_normed"):
    """Every pattern's score row over displacements k_lo .. k_lo + n_shift - 1 from its base, by the CPU oracle."""
    return [oracle.match_template(dst.data[0, b + k_lo:b + k_lo + n_shift + p.shape[1] - 1], p[0], method=method)[0]
            for b, p in zip(bases, patterns)]


# ---------------------------------------------------------------------------------------------- ragged synthetic groups
SHAPES = [(1, 1), (2, 63), (7, 64), (9, 65), (33, 1023), (3, 4097), (16, 70001)]      # (rows, shifts) of the groups of one call


def ragged_groups(method, seed=0):
    """One call's worth of synthetic rows: a curve buffer in which the rows of the SHAPES groups lie interleaved at odd offsets,
    the (curve_off, weight) rows in group order and the (first_row, n_rows, n_shift) groups.  Weights: equal, 1/3 and 0 by turns.
    Planted: in the (33, 1023) group an exact tie of the joint row across a workgroup boundary (indices 511 and 512: the better
    extremum of the group twice), in the (3, 4097) group the extremum in the last element twice over (4095 and 4096), and the
    (9, 65) group is all ones.  Values are float32 in [0.25, 0.75) ('sqdiff_normed') or [-0.5, 0) ('ccoeff_normed')."""
    rng = np.random.default_rng(seed)
    n_rows = sum(m for m, _n in SHAPES)
    # interleave: rows are laid out in an order that mixes the groups, each one an odd number of floats behind the last
    order = rng.permutation(n_rows)
    shift_of = np.concatenate([[n] * m for m, n in SHAPES])
    offs = np.zeros(n_rows, np.int64)
    at = 1
    for r in order:
        offs[r] = at
        at += int(shift_of[r]) + 1 + 2 * int(rng.integers(0, 3))
        at += (at + 1) % 2                                             # keep every offset odd
    curves = rng.random(at, dtype=np.float32) * np.float32(0.5) + np.float32(0.25 if method == "sqdiff_normed" else -0.5)
    best = np.float32(0.125 if method == "sqdiff_normed" else 0.875)   # beyond every random value, and every weight keeps that order
    rows, groups, first = [], [], 0
    for g, (m, n) in enumerate(SHAPES):
        kinds = [1.0 / m, 1.0 / 3.0, 0.0]
        w = [kinds[(g + i) % 3] if m > 2 else 1.0 / m for i in range(m)]
        if (m, n) == (9, 65):
            for i in range(m):
                curves[offs[first + i]:offs[first + i] + n] = 1.0
        if (m, n) == (33, 1023):
            for i in range(m):
                curves[offs[first + i] + 511] = curves[offs[first + i] + 512] = best
        if (m, n) == (3, 4097):
            for i in range(m):
                curves[offs[first + i] + 4095] = curves[offs[first + i] + 4096] = best
        rows += [(int(offs[first + i]), w[i]) for i in range(m)]
        groups.append((first, m, n))
        first += m
    return curves, rows, groups
