"""What tests/test_drift_host.py and tests/test_drift_gpu.py share: synthetic rows and offset tables for sushi_hip_drift_reduce, the
smallest shapes at which the kernel can go wrong, and the end-to-end scenario (a source retimed by 2001/2000)."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

DB = 2                      # csrc/drift_core.hpp DRIFT_DB: candidates per block
ROWS_AHEAD = 4              # csrc/sushi_drift.hip: rows whose loads are in flight together (at most)
ROWS = (1, 3, 4, 5, 9)                                  # either side of ROWS_AHEAD, and two rounds of it + 1
# 2048 * 8 + 77 shifts (9 items of 2048) x 229 blocks of candidates: from 2048 items of 2048 shifts on a workgroup takes eight indices per thread
LARGE_SHIFTS, LARGE_DRIFTS = 2048 * 8 + 77, DB * 228 + 1
SHIFTS = (1, 63, 64, 65, 257, 513, 2049)
DRIFTS = (1, DB - 1, DB, DB + 1, 2 * DB + 3)
KINDS = ("zero", "negative", "positive", "mixed")

Case = namedtuple("Case", "name curves rows n_shift offsets expect")      # rows: [(curve_off, weight)]; expect: (drift, index) or None


def _layout(rng, n_rows, n_shift, method):
    """A curve buffer holding n_rows rows of n_shift floats at odd offsets with gaps between them; values float32 in [0.25, 0.75)
    ('sqdiff_normed') or [-0.5, 0) ('ccoeff_normed'), so that 0.125 / 0.875 and 0.0 are beyond every random value."""
    offs, at = [], 1
    for _ in range(n_rows):
        offs.append(at)
        at += n_shift + 1 + 2 * int(rng.integers(0, 3))
        at += (at + 1) % 2
    curves = rng.random(at, dtype=np.float32) * np.float32(0.5) + np.float32(0.25 if method == "sqdiff_normed" else -0.5)
    return curves, offs[::-1] if n_rows % 2 else offs       # (not always ascending)


def _weights(n_rows, turn):
    kinds = [1.0 / n_rows, 1.0 / 3.0, 0.0]
    return [kinds[(turn + i) % 3] if n_rows > 2 else 1.0 / n_rows for i in range(n_rows)]


def _offsets(rng, kind, n_drifts, n_rows, n_shift):
    """Offsets of one sign pattern whose reach (max(0, max o) + max(0, max -o)) stays below n_shift."""
    room = min(9, (n_shift - 1) // 2)
    if kind == "zero" or room == 0:
        return np.zeros((n_drifts, n_rows), np.int32)
    lo, hi = {"negative": (-room, 0), "positive": (1, room + 1), "mixed": (-room, room + 1)}[kind]
    return rng.integers(lo, hi, size=(n_drifts, n_rows)).astype(np.int32)


def _best(method):
    return np.float32(0.125 if method == "sqdiff_normed" else 0.875)


def grid_cases(method, seed=5):
    """Every n_shift of SHIFTS with every E of ROWS, the candidate counts and offset kinds taken by turns, so that each value of
    DRIFTS and KINDS meets each n_shift; weights 1/E, 1/3 and 0 by turns."""
    rng = np.random.default_rng(seed)
    out, turn = [], 0
    for n_shift in SHIFTS:
        for n_rows in ROWS:
            n_drifts, kind = DRIFTS[turn % len(DRIFTS)], KINDS[(turn // 2) % len(KINDS)]
            curves, offs = _layout(rng, n_rows, n_shift, method)
            out.append(Case("grid_E%d_n%d_D%d_%s" % (n_rows, n_shift, n_drifts, kind), curves,
                            list(zip(offs, _weights(n_rows, turn))), n_shift, _offsets(rng, kind, n_drifts, n_rows, n_shift), None))
            turn += 3
    return out


def special_cases(method, seed=6):
    rng = np.random.default_rng(seed)
    best = _best(method)
    out = []
    # a candidate whose valid range is the single index 30, among candidates with wide ranges; planted: the best value on its line
    curves, offs = _layout(rng, 3, 65, method)
    o = np.array([[0, 0, 0], [-30, 34, 0], [1, -1, 2], [0, 0, 0], [2, 2, 2]], np.int32)
    for e in range(3):
        curves[offs[e] + 30 + int(o[1, e])] = best
    out.append(Case("single_index_range", curves, [(offs[e], 1.0 / 3.0) for e in range(3)], 65, o, (1, 30)))
    # ranges that end inside the last item (1200 shifts: items of 512; hi = 1100 and 1190), the best in the last valid element
    curves, offs = _layout(rng, 4, 1200, method)
    o = np.array([[100, 0, 3, -2], [0, 0, 0, 0], [10, -7, 0, 1]], np.int32)
    for e in range(4):
        curves[offs[e] + 1099 + int(o[0, e])] = best
    out.append(Case("range_ends_in_last_item", curves, [(offs[e], 0.25) for e in range(4)], 1200, o, (0, 1099)))
    # a tie inside one candidate across a workgroup boundary (511 | 512), and the same offsets again as a later candidate: the first
    # candidate and the first index win
    curves, offs = _layout(rng, 5, 1025, method)
    o = np.array([[3, -3, 0, 1, 2], [0, 0, 0, 0, 0], [-4, 4, 1, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0]], np.int32)
    for e in range(5):
        curves[offs[e] + 511] = curves[offs[e] + 512] = best
    out.append(Case("tie_across_workgroups_and_candidates", curves, list(zip(offs, _weights(5, 1))), 1025, o, (1, 511)))
    # the same line reached by two candidates at different indices: offsets all +2 at index j are offsets all 0 at index j + 2
    curves, offs = _layout(rng, 3, 257, method)
    o = np.array([[1, 0, 1], [2, 2, 2], [0, 0, 0]], np.int32)
    for e in range(3):
        curves[offs[e] + 100] = best
    out.append(Case("one_line_two_candidates", curves, [(offs[e], 1.0 / 3.0) for e in range(3)], 257, o, (1, 98)))
    # rows of 0.0 and -0.0 among values that are worse: the zeros tie, the first wins, and its own bits come back
    curves, offs = _layout(rng, 2, 64, method)
    curves[offs[0]:offs[0] + 64][[20, 21, 40]] = [-0.0, 0.0, -0.0]
    curves[offs[1]:offs[1] + 64][[21, 22, 41]] = [0.0, -0.0, 0.0]
    o = np.array([[0, 3], [0, 1], [0, 1], [0, 0]], np.int32)
    out.append(Case("signed_zeros", curves, [(offs[0], 0.5), (offs[1], 0.5)], 64, o, (1, 20)))
    # all ones: every (candidate, index) ties; the first candidate's range starts at 5
    curves, offs = _layout(rng, 9, 513, method)
    curves[:] = 1.0
    o = _offsets(rng, "mixed", 2 * DB + 3, 9, 513)
    o[0] = [-5, 0, 1, 2, 3, 4, 0, -1, 2]
    out.append(Case("all_ones", curves, list(zip(offs, _weights(9, 0))), 513, o, (0, 5)))
    return out


def large_case(method, seed=7):
    """Items of eight indices per thread (LARGE_SHIFTS x LARGE_DRIFTS), the last item cut short, the last block one candidate; the
    best planted in the last candidate's last valid element."""
    rng = np.random.default_rng(seed)
    curves, offs = _layout(rng, 3, LARGE_SHIFTS, method)
    o = _offsets(rng, "mixed", LARGE_DRIFTS, 3, LARGE_SHIFTS)
    o[-1] = [40, -3, 0]                                     # (a spread no random candidate has: nothing else reaches the planted line)
    for e in range(3):
        curves[offs[e] + LARGE_SHIFTS - 41 + int(o[-1, e])] = _best(method)
    return Case("large_items", curves, [(offs[0], 1.0 / 3.0), (offs[1], 1.0 / 3.0), (offs[2], 1.0 / 3.0)], LARGE_SHIFTS, o,
                (LARGE_DRIFTS - 1, LARGE_SHIFTS - 41))


def rows_of(case):
    return [case.curves[o:o + case.n_shift] for o, _w in case.rows], [w for _o, w in case.rows]


# ---------------------------------------------------------------------------------------------- the end-to-end scenario
# A 60 s stream at 12 kHz and the same stream read 2001/2000 times as slowly: the event at source instant t is found at t * 2001 /
# 2000 of the destination, the shift grows by 1/2000 s per second.  Twelve events of 1.5 s spread over the programme, window 0.5 s,
# rates out to 1e-3.
RATE = 12000
SECONDS = 60
SPEED = Fraction(2001, 2000)
EVENT_LENGTH = 1.5
EVENT_STARTS = [2.0 + 5.0 * i for i in range(12)]           # 2.0 .. 57.0: a half span of 27.5 s, 661 candidates
WINDOW = 0.5
MAX_RATE = 1e-3
TRUE_RATE = 1.0 / 2000
NEIGHBOURHOOD = 16          # samples either side of an event's true place in which its own minimum is looked for
# |event on the line - the event's own minimum near its true place| in samples: <= 0.5 from half a grid step at the farthest event,
# <= 0.5 from rint, <= 1 from the two truncations (retimed's read positions, _get_sample_for_time)
EVENT_TOLERANCE = 2


def drift_streams(sample_type="uint8"):
    """(destination, source) WavStreams of the scenario."""
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    src = WavStream.from_samples(synth.make_dst_pcm(SECONDS, RATE, seed=41), RATE, sample_type=sample_type)
    return src.retimed(SPEED), src


def true_place(dst, start):
    """The destination sample (row index) at which the event that starts at source instant `start` truly lies, as a real number."""
    return start * RATE * float(SPEED) + dst.padding_size
