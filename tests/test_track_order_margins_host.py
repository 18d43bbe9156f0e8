"""Ordered margins without a GPU: the NumPy restatement of sushi_hip_track_order_margins (sushi_amd/track.py
track_ordered_margins_host) against a brute force over all ordered paths, its four stated facts (the exact path minimum, the
reversal identity, consistency with the total, and the plain margins where no back binds), the suffix minimum and its ties, the
edges of the backs and of the guard window, the kernels' own header compiled for the CPU
(tests/host_track_order_margins_check.cpp, a program of its own under AddressSanitizer + UBSan), the entry points' argument checks,
and the two scenarios: two explanations planted and mirrored, and the decoys on the CPU oracle."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import track_cases
import track_order_cases as ocases
import track_order_margin_cases as cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, joint, track
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP, ANY = -32768, -1


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("track_order_margins_check")), "host_track_order_margins_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_track_order_margins_check.cpp"), "-o", exe])
    return exe


def _np_reductions(got, guard):
    """through, best, alt and their indices from got.marginals by NumPy, with the first-index rule."""
    E, n = got.marginals.shape
    for e in range(E):
        M, s = got.marginals[e], int(got.shifts[e])
        assert _bits64(got.through[e]) == _bits64(M[s])
        assert got.best_arg[e] == int(np.argmin(M)) and _bits64(got.best[e]) == _bits64(M[int(np.argmin(M))])
        outside = [j for j in range(n) if abs(j - s) > guard[e]]
        if outside:
            at = min(outside, key=lambda j: (M[j], j))
            assert got.alt_arg[e] == at and _bits64(got.alt[e]) == _bits64(M[at]), e
        else:
            assert got.alt_arg[e] == -1 and got.alt[e] == np.inf
    assert got.through.dtype == got.best.dtype == got.alt.dtype == got.c_min.dtype == np.float64
    assert got.best_arg.dtype == got.alt_arg.dtype == np.int32 and got.D.shape == got.marginals.shape


# ---------------------------------------------------------------------------------------------- fact 1: the exact path minimum
def _u(rows, weights, method, e, j):
    return float(weights[e]) * (-float(rows[e][j]) if method == "ccoeff_normed" else float(rows[e][j]))


def _cheapest(c, a, b, r, lam, mu, back):
    """What the step from shift a of one event to shift b of the next adds to c: the cheapest allowed choice of a move's price
    (nothing for a == b) and lam, a jump existing iff b >= a - back; inf where the step can be made neither way."""
    d = abs(a - b)
    choices = []
    if back < 0 or b >= a - back:
        choices.append(c + lam)
    if d == 0:
        choices.append(c)
    elif d <= r:
        choices.append(c + mu * float(d))
    return min(choices) if choices else float("inf")


def _through_path(rows, weights, lams, mu, reach, back, method, path, e):
    """(prefix cost of events 0 .. e, accumulated forwards) + (suffix cost of events E-1 .. e+1, accumulated backwards, and the step
    into it from event e; u_e is not added again)."""
    E = len(rows)
    p = _u(rows, weights, method, 0, path[0])
    for i in range(1, e + 1):
        p = _u(rows, weights, method, i, path[i]) + _cheapest(p, path[i - 1], path[i], reach[i], lams[i], mu, back[i])
    if e == E - 1:
        return p
    c = _u(rows, weights, method, E - 1, path[E - 1])
    for i in range(E - 2, e, -1):
        c = _u(rows, weights, method, i, path[i]) + _cheapest(c, path[i], path[i + 1], reach[i + 1], lams[i + 1], mu, back[i + 1])
    return p + _cheapest(c, path[e], path[e + 1], reach[e + 1], lams[e + 1], mu, back[e + 1])


@pytest.mark.parametrize("method", METHODS)
def test_every_marginal_is_the_minimum_over_all_ordered_paths_through_it(method):
    """E <= 4 rows over n <= 7 shifts, random float32 rows and dyadic ones with planted ties, reaches 0 .. 3, backs from {-1, 0, 1, 2,
    n}, penalties per row including 0, weights including 0: every M_e[j] is bitwise the minimum over all n^E paths with s_e = j whose
    jumps obey the backs; through, best and alt are NumPy's on those rows; some back binds."""
    rng = np.random.default_rng(23)
    sign = -1.0 if method == "ccoeff_normed" else 1.0
    seen_alt = seen_none = seen_bound = False
    for trial, (E, n) in enumerate([(1, 1), (1, 5), (2, 3), (2, 7), (3, 5), (3, 6), (4, 4), (4, 7), (4, 7), (3, 7), (4, 6), (4, 5)]):
        if trial % 2:       # dyadic values: every sum exact, ties are real ties (never 0: a weighted cost keeps its sign)
            rows = [(sign * rng.integers(1, 9, n) / 8.0).astype(np.float32) for _ in range(E)]
            lams = [(0.25, 0.0, 0.125, 0.5, 1.0)[int(k)] for k in rng.integers(0, 5, E)]
            mu = (0.0, 0.125, 0.25)[trial % 3]
        else:
            rows = [(sign * (rng.random(n, dtype=np.float32) * np.float32(0.875) + np.float32(0.0625))).astype(np.float32) for _ in range(E)]
            lams = [(0.3, 1.0 / 3.0, 0.05, 0.0)[int(k)] for k in rng.integers(0, 4, E)]
            mu = (1e-2, 0.0, 0.07)[trial % 3]
        weights = [(1.0, 0.0, 2.5, 1.0 / 3.0)[(e + trial) % 4] for e in range(E)]
        weights[0] = weights[0] or 1.0
        reach = [int(k) for k in rng.integers(0, 4, E)]
        back = [(ANY, 0, 1, 2, n)[int(k)] for k in rng.integers(0, 5, E)]
        guard = [int(k) for k in rng.integers(0, n + 1, E)]
        got = track.track_ordered_margins_host(rows, weights, lams, mu, reach, back, guard, method)
        reach[0] = 0
        paths = list(itertools.product(range(n), repeat=E))
        for e in range(E):
            costs = [_through_path(rows, weights, lams, mu, reach, back, method, p, e) for p in paths]
            for j in range(n):
                want = min(c for c, p in zip(costs, paths) if p[e] == j)
                assert _bits64(got.marginals[e, j]) == _bits64(want), (E, n, e, j)
        _np_reductions(got, guard)
        assert (_bits64(got.marginals[E - 1]) == _bits64(got.D[E - 1])).all()
        fwd = track.track_ordered_host(rows, weights, lams, mu, reach, back, method)
        assert fwd.shifts.tolist() == got.shifts.tolist() and _bits64(fwd.cost) == _bits64(got.cost)
        assert (fwd.moves == got.moves).all() and (fwd.prefix_arg == got.prefix_arg).all()
        free = track.track_ordered_margins_host(rows, weights, lams, mu, reach, ANY, guard, method)
        seen_bound |= bool((free.marginals < got.marginals).any())
        seen_alt |= bool((got.alt_arg >= 0).any())
        seen_none |= bool((got.alt_arg < 0).any())
    assert seen_alt and seen_none and seen_bound


# ---------------------------------------------------------------------------------------------- facts 2 - 4, synthetic sequences
@pytest.fixture(scope="module", params=METHODS)
def sequences(request):
    out = {}
    for E, n, reach in track_cases.SHAPES:
        curves, rows, weights, lams, rs, mu, back, guard = cases.sequence(E, n, reach, request.param, seed=3)
        rows = track_cases.rows_of(curves, rows, n)
        out[(E, n, reach)] = (rows, weights, lams, rs, mu, back, guard,
                              track.track_ordered_margins_host(rows, weights, lams, mu, rs, back, guard, request.param))
    return request.param, out


def _path_terms(got, rows, weights, lams, mu):
    """S of the bound |through_e - cost| <= 6 E 2^-53 S: the sum of the absolute values of the optimal path's terms."""
    total = 0.0
    for e, s in enumerate(got.shifts):
        total += abs(float(weights[e]) * float(rows[e][s]))
        if e:
            word = int(got.moves[e, s])
            total += float(lams[e]) if word == JUMP else float(mu) * abs(word)
    return total


@pytest.mark.parametrize("shape", track_cases.SHAPES)
def test_reversal_and_consistency_with_the_total(sequences, shape):
    method, table = sequences
    rows, weights, lams, rs, mu, back, guard, got = table[shape]
    E = shape[0]
    # reversal: c_min_0 is the ordered forward pass's total on the reversed sequence, every row flipped end to end
    rev = track.track_ordered_host([r[::-1].copy() for r in rows[::-1]], weights[::-1], [0.0] + [lams[E - i] for i in range(1, E)], mu,
                                   [0] + [rs[E - i] for i in range(1, E)], [ANY] + [back[E - i] for i in range(1, E)], method)
    assert rev.cost == got.c_min[0]
    assert (rev.row_min[::-1] == got.c_min).all()
    # consistency: best <= through and best <= alt exactly; through is the total up to summation order
    assert (got.best <= got.through).all() and (got.best <= got.alt).all()
    S = _path_terms(got, rows, weights, lams, mu)
    assert (np.abs(got.through - got.cost) <= 6 * E * 2.0 ** -53 * S).all(), (np.abs(got.through - got.cost).max(), S)
    assert all(_bits64(got.marginals[e, got.best_arg[e]]) == _bits64(got.best[e]) for e in range(E))
    _np_reductions(got, guard)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", track_cases.SHAPES)
def test_without_a_limit_they_are_the_plain_margins(shape, method):
    """Fact 4: every used back BACK_ANY or >= n_shift - 1, and one penalty: every output is track_margins_host's, bit for bit."""
    E, n, reach = shape
    curves, rows, weights, lam, rs, mu = track_cases.sequence(E, n, reach, method, seed=3)
    rows = track_cases.rows_of(curves, rows, n)
    guard = cases.guards(E, n)
    want = track.track_margins_host(rows, weights, lam, mu, rs, guard, method)
    for back in (ANY, None, [ANY] + [(ANY, n - 1, n + 7, 2 ** 31 - 1)[e % 4] for e in range(1, E)]):
        got = track.track_ordered_margins_host(rows, weights, lam, mu, rs, back, guard, method)
        for name in track.TrackMarginsHost._fields:
            a, b = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name


# ---------------------------------------------------------------------------------------------- the suffix minimum
def _suffix_loop(C):
    """The definition, written out: walking down, a value at or below the running minimum replaces it."""
    out, run = [0.0] * len(C), None
    for t in range(len(C) - 1, -1, -1):
        if run is None or float(C[t]) <= run:
            run = float(C[t])
        out[t] = run
    return np.array(out, np.float64)


def test_suffix():
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 513, 1024):
        for C in (rng.random(n), np.round(rng.random(n) * 4) / 4, np.arange(n, dtype=np.float64), np.arange(n, 0, -1.0), np.zeros(n)):
            assert (_bits64(track._suffix(C)) == _bits64(_suffix_loop(C))).all()
    # equal minima on both sides of a wave's, a round's and a work item's boundary
    for at in (256, 512):
        C = rng.random(1024) * 0.25 + 0.5
        C[[at - 1, at]] = 0.25
        S = track._suffix(C)
        assert (S[:at + 1] == 0.25).all() and (S[at + 1:] > 0.25).all()
    # a decreasing row is its own last value everywhere; an increasing one is itself
    down, up = np.arange(9, 0, -1.0), np.arange(1.0, 10.0)
    assert track._suffix(down).tolist() == [1.0] * 9 and track._suffix(up).tolist() == up.tolist()
    # of 0.0 and -0.0 the lower index's zero is kept
    for C, want in (([0.0, -0.0, 1.0], [0.0, -0.0, 1.0]), ([-0.0, 0.0, 1.0], [-0.0, 0.0, 1.0]), ([1.0, -0.0, 0.0], [-0.0, -0.0, 0.0])):
        assert (_bits64(track._suffix(np.array(C))) == _bits64(np.array(want))).all()
    assert track._reach_from(5, 2).tolist() == [0, 0, 0, 1, 2] and track._reach_from(3, ANY).tolist() == [0, 0, 0]
    assert track._reach_from(3, 0).tolist() == [0, 1, 2] and track._reach_from(3, 2 ** 31 - 1).tolist() == [0, 0, 0]


def test_negative_zero_travels_through_the_suffix_minimum():
    """A last row of zeros of both signs (and, under ccoeff or with weight 0, of the other signs): S keeps the sign of the zero at the
    lowest index, a penalty of -0.0 is a valid 0 and leaves jumpB with the sign of S, and M is D + B with exactly that B."""
    rows = [np.array([0.5, 0.25, 0.75], np.float32), np.array([0.0, -0.0, 0.0], np.float32)]
    for method in METHODS:
        for w in ([1.0, 0.0], [1.0, 1.0]):
            got = track.track_ordered_margins_host(rows, w, [0.0, -0.0], 0.0, 0, [ANY, 1], 0, method)
            u1 = np.float64(w[1]) * (-rows[1].astype(np.float64) if method == "ccoeff_normed" else rows[1].astype(np.float64))
            S = _suffix_loop(u1)
            assert (_bits64(track._suffix(u1)) == _bits64(S)).all() and _bits64(S[0]) == _bits64(u1[0])
            jump = S[[0, 0, 1]] + (-0.0)                    # back 1: t' = 0, 0, 1
            assert (_bits64(jump) == _bits64(S[[0, 0, 1]])).all()
            B = np.where(u1 <= jump, u1, jump)
            assert (_bits64(got.marginals[0]) == _bits64(got.D[0] + B)).all()
            assert _bits64(got.c_min[1]) == _bits64(S[0])


# ---------------------------------------------------------------------------------------------- the backs' edges, ties
def test_back_zero_at_index_zero_and_a_back_beyond_the_axis():
    a = np.array([0.5, 0.9, 0.9, 0.9], np.float32)
    b = np.array([0.9, 0.9, 0.9, 0.1], np.float32)
    c = np.array([0.1, 0.9, 0.9, 0.9], np.float32)
    # back 0: a jump never lowers the shift.  Out of (0, 0) every index of row 1 can be reached; out of (1, 3) only index 3 of row 2
    got = track.track_ordered_margins_host([a, b, c], [1.0] * 3, 0.125, 0.0, 0, [ANY, 0, 0], 0)
    u = lambda r: r.astype(np.float64)
    S2 = track._suffix(u(c))
    C1 = u(b) + np.where(u(c) <= S2 + 0.125, u(c), S2 + 0.125)         # t' = j: the suffix from j on
    assert (_bits64(got.marginals[1]) == _bits64(got.D[1] + np.where(u(c) <= S2 + 0.125, u(c), S2 + 0.125))).all()
    S1 = track._suffix(C1)
    assert _bits64(got.c_min[1]) == _bits64(S1[0]) and _bits64(got.c_min[2]) == _bits64(np.float64(np.float32(0.1)))
    # index 0 of row 0 sees the whole of row 1; index 3 sees its index 3 alone
    B0 = np.where(C1 <= S1 + 0.125, C1, S1 + 0.125)
    assert (_bits64(got.marginals[0]) == _bits64(got.D[0] + B0)).all()
    # row 2's 0.1 at index 0 lies below row 1's 0.1 at index 3 and cannot be jumped to from there: the path stays at 0
    assert got.shifts.tolist() == [0, 0, 0] and got.cost == float(np.float32(0.1)) + (float(np.float32(0.9)) + 0.5)
    assert got.marginals[1, 3] > got.marginals[1, 0]
    # a back beyond the axis (and INT32_MAX) is no limit
    free = track.track_ordered_margins_host([a, b, c], [1.0] * 3, 0.125, 0.0, 0, ANY, 0)
    for back in (3, 4, 1000, 2 ** 31 - 1):
        got = track.track_ordered_margins_host([a, b, c], [1.0] * 3, 0.125, 0.0, 0, [ANY, back, back], 0)
        assert got.marginals.tobytes() == free.marginals.tobytes() and got.shifts.tolist() == free.shifts.tolist() == [0, 3, 0]


def test_a_tie_between_moving_and_jumping_moves():
    """nearB == jumpB: B has nearB's bits.  Under ccoeff u_1 = [0.0, -0.0]; S_1 = [0.0, -0.0]; without a limit and with penalty 0 jumpB =
    S_1[0] + 0.0 = +0.0 at both indices, and nearB[1] = -0.0 ties with it: C_0[1] = u_0[1] + B_0[1] with u_0 = -0.0 is -0.0 only if
    the tie took nearB."""
    last = np.array([-0.0, 0.0], np.float32)
    u1 = -last.astype(np.float64)
    S = track._suffix(u1)
    assert (_bits64(u1) == _bits64(np.array([0.0, -0.0]))).all() and (_bits64(S) == _bits64(np.array([0.0, -0.0]))).all()
    trace = []
    track.track_ordered_margins_host([np.array([0.0, 0.0], np.float32), last], [1.0, 1.0], [0.0, 0.0], 0.0, 0, ANY, 0, "ccoeff_normed",
                                     _trace=trace)
    C0 = [c for e, c, _s in trace if e == 0][0]
    assert (_bits64(C0) == _bits64(np.array([0.0, -0.0]))).all()          # -0.0 + (+0.0) = +0.0;  -0.0 + (-0.0) = -0.0
    # a penalty above 0: nothing ties, and the jump is taken where it is cheaper
    got = track.track_ordered_margins_host([np.array([0.5, 0.5], np.float32), np.array([0.75, 0.25], np.float32)], [1.0, 1.0],
                                           [0.0, 0.125], 0.0, 0, [ANY, 0], 0)
    assert got.marginals[0].tolist() == [0.5 + 0.375, 0.5 + 0.25] and got.c_min.tolist() == [0.75, 0.25]


def test_guard_edges():
    lone = np.array([0.5, 0.25, 0.9, 0.1, 0.9, 0.25, 0.5], np.float32)
    one = lambda g: track.track_ordered_margins_host([lone], [1.0], 0.5, 0.0, 0, 0, g)
    got = one(1)                                        # E = 1: M is u itself.  s = 3; equal values on both sides: the first index
    assert got.shifts.tolist() == [3] and (_bits64(got.marginals[0]) == _bits64(lone.astype(np.float64))).all()
    assert (got.alt_arg.tolist(), got.alt.tolist(), got.best_arg.tolist()) == ([1], [0.25], [3])
    assert _bits64(got.through[0]) == _bits64(np.float64(np.float32(0.1))) == _bits64(got.c_min[0])
    assert one(0).alt_arg.tolist() == [1]
    got = one(2)                                        # the window covers 1 .. 5: 0.5 at 0 before 0.5 at 6
    assert (got.alt_arg.tolist(), got.alt.tolist()) == ([0], [0.5])
    for g in (3, 7, 8, 2 ** 31 - 1):                    # the window ends at both axis ends, or beyond: nothing outside
        got = one(g)
        assert got.alt_arg.tolist() == [-1] and got.alt.tolist() == [np.inf] and got.best_arg.tolist() == [3]
    got = track.track_ordered_margins_host([lone, lone], [1.0, 1.0], 0.5, 0.0, 0, 0, [0, 3])
    assert got.alt_arg.tolist() == [1, -1] and got.shifts.tolist() == [3, 3]
    for bad in (-1, [1], [1, 2, 3], "wide", [0, None], 2 ** 31):
        with pytest.raises(SushiError):
            track.track_ordered_margins_host([lone, lone], [1.0, 1.0], 0.5, 0.0, 0, 0, bad)
    for kw in (dict(back=-2), dict(back=[0]), dict(penalties=[0.0, -1.0]), dict(penalties=[0.0, float("nan")]), dict(reach=1025)):
        args = dict(penalties=0.5, reach=0, back=0)
        args.update(kw)
        with pytest.raises(SushiError):
            track.track_ordered_margins_host([lone, lone], [1.0, 1.0], args["penalties"], 0.0, args["reach"], args["back"], 0)


# ---------------------------------------------------------------------------------------------- two explanations, mirrored
def test_plain_margins_understate_what_the_ordered_model_gives():
    lam, mu, reach, guard = cases.PLANT_PENALTY, cases.PLANT_STEP_COST, cases.PLANT_REACH, cases.PLANT_GUARD
    rows = cases.planted()
    plain = track.track_margins_host(rows, [1.0] * 6, lam, mu, reach, guard)
    for back, want in ((ANY, cases.PLANT_MARGINS_PLAIN), (cases.PLANT_BACK, cases.PLANT_MARGINS_ORDERED)):
        got = track.track_ordered_margins_host(rows, [1.0] * 6, lam, mu, reach, back, guard)
        margin = got.alt - got.through
        assert got.shifts.tolist() == [cases.PLANT_HERE] * 6 and got.alt_arg.tolist() == [cases.PLANT_THERE] * 6
        assert np.abs(margin - np.array(want)).max() < 1e-6, (back, margin)
    free = track.track_ordered_margins_host(rows, [1.0] * 6, lam, mu, reach, ANY, guard)
    assert free.marginals.tobytes() == plain.marginals.tobytes() and free.alt.tobytes() == plain.alt.tobytes()
    assert np.abs((plain.alt - plain.through) - np.array(cases.PLANT_MARGINS_PLAIN)).max() < 1e-6
    # without the anchor the run has two explanations 6 x 0.02 apart, whatever the back
    for back in (ANY, cases.PLANT_BACK):
        got = track.track_ordered_margins_host(cases.planted(anchor=None), [1.0] * 6, lam, mu, reach, back, guard)
        assert np.abs((got.alt - got.through) - cases.PLANT_MARGIN_NO_ANCHOR).max() < 1e-6 and got.alt_arg.tolist() == [cases.PLANT_THERE] * 6


# ---------------------------------------------------------------------------------------------- the kernels' header on the CPU
EXPECTED_RC = {   # case of host_track_order_margins_check validate -> what stage_order_margins returns
    "good": 0, "good_ccoeff": 0, "null_rows": -1, "null_reach": -1, "null_guard": -1, "null_mem": -1, "method_2": -1, "no_rows": -1,
    "no_shift": -1, "empty_curves": -1, "shift_beyond_curves": -1, "rows_end_at_sequence_end": 0, "rows_past_sequence_end": -1,
    "row0_negative": -1, "no_total": -1, "rows_sum_overflows_int": -1, "row_ends_at_curves_end": 0, "row_one_past_curves_end": -1,
    "row_at_int64_max": -1, "weight_nan": -1, "weight_negative": -1, "step_cost_nan": -1, "step_cost_negative": -1, "reach_1025": -1,
    "reach_negative": -1, "reach_entry_0_is_ignored": 0, "reach_of_the_row_after_the_call": -1,
    "reach_after_the_last_row_is_not_read": 0, "guard_negative": -1, "null_back": -1, "back_all_any": 0, "back_all_zero": 0,
    "back_int_max": 0, "back_minus_two": -1, "back_int_min": -1, "back_entry_0_is_ignored": 0, "back_of_the_row_after_the_call": -1,
    "back_after_the_last_row_is_not_read": 0, "null_penalty": -1, "penalty_nan": -1, "penalty_inf": -1, "penalty_negative": -1,
    "penalty_neg_zero": 0, "penalty_entry_0_is_ignored": 0, "penalty_of_the_row_after_the_call": -1,
    "penalty_after_the_last_row_is_not_read": 0, "workspace_exact": 0, "workspace_short": -4, "workspace_of_the_plain_margins": -4,
    "workspace_misaligned": -2, "workspace_misaligned_and_short": -2, "bad_back_before_workspace": -1,
    "bad_penalty_before_alignment": -1, "bad_guard_and_back_before_workspace": -1}


def test_stage_order_margins_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = dict(l.split() for l in lines[:len(EXPECTED_RC)])
    assert {k: int(v) for k, v in got.items()} == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    # one set of partial records (36 bytes a workgroup), then three arrays of one entry per work item (8, 4 and 8 bytes), each padded
    # to 256 bytes
    assert rest[0] == "bytes 1024 1024 %d 0 0 0" % (16896 + 3840 + 2048 + 3840)
    assert rest[1] == "from 5 1 0 0 0 0 0"
    assert rest[2] == "facts_one rc=0 per=2 items=1 grid=1 first=1 set=256 offsets=(256,512,768) bytes=1024"
    assert rest[3] == "facts_513 rc=0 per=2 items=2 grid=2 first=1 set=256 offsets=(256,512,768) bytes=1024"
    assert rest[4] == "facts_240001 rc=0 per=2 items=469 grid=469 first=1 set=16896 offsets=(16896,20736,22784) bytes=26624"
    assert rest[5] == "facts_2880001 rc=0 per=8 items=1407 grid=1407 first=1 set=50688 offsets=(50688,61952,67584) bytes=78848"
    # 2^20 items of 2048: 20 bytes each behind a set of 2048 partial records
    assert rest[6] == "facts_int32_max rc=0 per=8 items=1048576 grid=2048 first=1 set=73728 offsets=(73728,8462336,12656640) " \
        "bytes=%d" % (73728 + 20 * 2 ** 20)
    assert len(rest) == 7


def _run_check(check, tmp_path, method, mu, n, split, curves, rows, reach, back, lams, guard, D, shifts):
    rt = np.array(rows, dtype=_native.JOINT_ROW_DTYPE)
    names = ("curves", "rows", "reach", "back", "penalty", "guard", "D", "shifts", "out")
    paths = [os.path.join(str(tmp_path), name) for name in names]
    for path, a in zip(paths, (curves, rt, np.array(reach, np.int32), np.array(back, np.int32), np.array(lams, np.float64),
                               np.array(guard, np.int32), np.ascontiguousarray(D, np.float64), np.array(shifts, np.int32))):
        a.tofile(path)
    subprocess.check_call([check, "pass", method.split("_")[0], float(mu).hex(), str(n), str(split)] + paths)
    raw = np.fromfile(paths[-1], np.uint8)
    E = len(rows)
    take = lambda a, b, dtype: raw[a:b].copy().view(dtype)
    through, best, alt, c_min = (take(8 * E * k, 8 * E * (k + 1), np.uint64) for k in range(4))
    best_arg, alt_arg = (take(32 * E + 4 * E * k, 32 * E + 4 * E * (k + 1), np.int32) for k in range(2))
    at = 40 * E
    M = take(at, at + 8 * E * n, np.uint64).reshape(E, n)
    C = take(at + 8 * E * n, at + 8 * E * n + 16 * n, np.uint64).reshape(2, n)
    S = take(at + 8 * E * n + 16 * n, at + 8 * E * n + 24 * n, np.uint64)
    assert raw.shape[0] == at + 8 * E * n + 24 * n
    return through, best, alt, c_min, best_arg, alt_arg, M, C, S


def _compare_with_host(check, tmp_path, method, mu, n, split, curves, rows, weights, reach, back, lams, guard):
    trace = []
    want = track.track_ordered_margins_host(track_cases.rows_of(curves, rows, n), weights, lams, mu, reach, back, guard, method,
                                            _trace=trace)
    through, best, alt, c_min, best_arg, alt_arg, M, C, S = _run_check(check, tmp_path, method, mu, n, split, curves, rows, reach, back,
                                                                       lams, guard, want.D, want.shifts)
    assert (through == _bits64(want.through)).all() and (best == _bits64(want.best)).all() and (alt == _bits64(want.alt)).all()
    assert (c_min == _bits64(want.c_min)).all() and best_arg.tolist() == want.best_arg.tolist()
    assert alt_arg.tolist() == want.alt_arg.tolist() and (M == _bits64(want.marginals)).all()
    by_row = {e: (c, s) for e, c, s in trace}
    E = len(rows)
    assert (C[0] == _bits64(by_row[0][0])).all() and (S == _bits64(by_row[0][1])).all()
    if E > 1:
        assert (C[1] == _bits64(by_row[1][0])).all()
    return want


@pytest.mark.parametrize("method", METHODS)
def test_the_header_on_the_cpu_equals_track_ordered_margins_host(check, tmp_path, method):
    """track_core.hpp's candidates, the margins' rules with order_margin_from and order_margin_jump, order_combine over the items'
    records and order_suffix_combine inside an item, grouped another way than the kernels group them and walked in two backward
    calls at an odd and an even boundary, run by a program of its own over the sequences of the GPU test but the longest."""
    bound = False
    for k, (E, n, reach) in enumerate(track_cases.SHAPES[:-1] + [(4, 1025, 600), (3, 5, 1024)]):
        curves, rows, weights, lams, rs, mu, back, guard = cases.sequence(E, n, reach, method, seed=3)
        for split in sorted({0, E // 2, (E // 2 + 1) % E}):
            want = _compare_with_host(check, tmp_path, method, mu, n, split, curves, rows, weights, rs, back, lams, guard)
        free = track.track_ordered_margins_host(track_cases.rows_of(curves, rows, n), weights, lams, mu, rs, ANY, guard, method)
        bound |= bool((free.marginals < want.marginals).any())
    assert bound


def test_the_header_on_the_cpu_on_cases_written_here(check, tmp_path):
    for method in METHODS:
        for at in (256, 512):
            a, b, c = cases.suffix_tie_rows(1024, at, method)
            curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b, np.zeros(1, np.float32), c])
            rows = [(1, 1.0), (1027, 1.0), (2052, 1.0)]
            # t' lands on each side of the tie: back 0 reads S at j itself, back 1 one below
            for back in (0, 1, at, ANY):
                _compare_with_host(check, tmp_path, method, 0.0, 1024, 1, curves, rows, [1.0] * 3, [0, 0, 0], [ANY, back, back],
                                   [0.0, 0.0625, 0.0625], [0, 5, 2000])
    # -0.0 through S under ccoeff with weight 0 and a penalty of -0.0; back 0 at index 0; a penalty of 0; the move / jump tie
    curves = np.array([0.5, -0.5, -0.5, -0.25, -0.25, -0.25, 0.5, 0.125, 0.75, 0.25, 0.5, 0.5, 0.5, 0.0, 0.25, 0.5, 1.0, 0.75, 0.75, 0.0,
                       -0.0, 0.0], np.float32)
    for method in METHODS:
        for rows, n, mu, reach, back, lams in (([(0, 0.0), (3, 0.0)], 3, 0.0, [0, 0], [ANY, ANY], [0.0, -0.0]),
                                               ([(0, 1.0), (19, 0.0)], 3, 0.0, [0, 0], [ANY, 1], [0.0, -0.0]),
                                               ([(0, 1.0), (19, 1.0)], 3, 0.0, [0, 0], [ANY, 0], [0.0, 0.0]),
                                               ([(6, 1.0), (10, 1.0)], 4, 0.0, [0, 0], [ANY, 0], [0.0, 0.0625]),
                                               ([(6, 1.0), (10, 1.0), (7, 0.5)], 4, 0.125, [0, 1, 1], [ANY, 0, 2], [0.0, 0.0, 0.25]),
                                               ([(14, 1.0), (17, 1.0)], 3, 0.25, [0, 1], [ANY, 0], [0.0, 0.5])):
            for split in range(len(rows)):
                _compare_with_host(check, tmp_path, method, mu, n, split, curves, rows, [w for _o, w in rows], reach, back, lams,
                                   [0] * len(rows))


# ---------------------------------------------------------------------------------------------- the entry points, no GPU
def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    assert {"sushi_hip_track_forward_ordered_keep", "sushi_hip_track_order_margins_bytes", "sushi_hip_track_order_margins"} <= \
        set(_native.declared_symbols())
    assert L.sushi_hip_abi_version() == 13
    assert L.sushi_hip_track_order_margins_bytes(1, 1) == 1024 and L.sushi_hip_track_order_margins_bytes(200, 240001) == 26624
    assert L.sushi_hip_track_order_margins_bytes(0, 5) == 0 and L.sushi_hip_track_order_margins_bytes(5, 0) == 0
    rows = np.array([(0, 1.0), (501, 0.0), (333, 2.5)], dtype=_native.JOINT_ROW_DTYPE)
    reach = np.array([0, 1024, 17, 3], np.int32)
    back = np.array([0, -1, 600, 0], np.int32)
    lams = np.array([0.5, 0.0, 2.0, 0.25], np.float64)
    guard = np.array([0, 120, 2 ** 31 - 1], np.int32)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(curves=P, n_curve=1000, rows=rows, reach=reach, back=back, guard=guard, lams=lams, n_rows=3, n_shift=499, method=0,
             step_cost=1e-3, row0=2, n_total=7, outs=(P,) * 10, M=P, mem=P, mem_bytes=1 << 16):
        return L.sushi_hip_track_order_margins(curves, n_curve, ptr(rows), ptr(reach), ptr(back), ptr(guard), n_rows, n_shift, method,
                                               ptr(lams), step_cost, row0, n_total, *outs, M, mem, mem_bytes, None)

    EINVAL, EALIGN = -1, -2
    assert call(mem_bytes=16) == _native.ENOSPACE                          # everything but the workspace is in order
    assert call(mem_bytes=16, M=None) == _native.ENOSPACE                  # M may be null
    for name in ("curves", "rows", "reach", "back", "guard", "lams", "mem"):
        assert call(**{name: None}) == EINVAL, name
    for k in range(10):                                                    # D, shifts, C, S, c_min, through, best, best_arg, alt, alt_arg
        assert call(outs=tuple(None if i == k else P for i in range(10))) == EINVAL, k
    assert call(method=2) == EINVAL and call(n_rows=0) == EINVAL and call(n_shift=0) == EINVAL and call(n_shift=1001) == EINVAL
    assert call(row0=-1) == EINVAL and call(row0=5) == EINVAL and call(n_total=0) == EINVAL
    for bad in (np.nan, np.inf, -1e-300):
        assert call(step_cost=bad) == EINVAL
        for at in (1, 2, 3):
            p = lams.copy()
            p[at] = bad
            assert call(lams=p) == EINVAL, (at, bad)
        p = lams.copy()
        p[0] = bad
        assert call(lams=p, mem_bytes=16) == _native.ENOSPACE              # entry 0 is not used
        p = lams.copy()
        p[3] = bad
        assert call(lams=p, row0=4, mem_bytes=16) == _native.ENOSPACE      # the call ends at the sequence's last row: not read
    for at, value in ((1, -2), (2, -(2 ** 31)), (3, -2)):
        b = back.copy()
        b[at] = value
        assert call(back=b) == EINVAL, (at, value)
    b = back.copy()
    b[0], b[1] = -2, 2 ** 31 - 1
    assert call(back=b, mem_bytes=16) == _native.ENOSPACE
    r = reach.copy()
    r[3] = 1025
    assert call(reach=r) == EINVAL and call(reach=r, row0=4, mem_bytes=16) == _native.ENOSPACE
    g = guard.copy()
    g[2] = -1
    assert call(guard=g) == EINVAL
    bad = rows.copy()
    bad["curve_off"][1] = 502
    assert call(rows=bad) == EINVAL
    assert call(mem=odd(128)) == EALIGN and call(mem_bytes=1023) == _native.ENOSPACE
    assert call(curves=odd(2)) == EALIGN and call(M=odd(4)) == EALIGN
    # D, shifts, C, S, c_min, through, best, best_arg, alt, alt_arg
    for k, off in enumerate((4, 2, 4, 4, 4, 4, 4, 2, 4, 2)):
        assert call(outs=tuple(odd(off) if i == k else P for i in range(10))) == EALIGN, k

    # forward_ordered_keep refuses what forward_ordered refuses
    def forward(fn, **kw):
        a = dict(curves=P, lams=lams[:3], back=back[:3], reach=reach[:3], outs=(P,) * 9, mem=P, mem_bytes=1 << 16, row0=2)
        a.update(kw)
        return fn(a["curves"], 1000, ptr(rows), ptr(a["reach"]), ptr(a["back"]), 3, 499, 0, ptr(a["lams"]), 1e-3, a["row0"], 7,
                  *a["outs"], a["mem"], a["mem_bytes"], None)

    for kw in (dict(mem_bytes=16), dict(curves=None), dict(lams=None), dict(back=None), dict(mem=odd(128)), dict(row0=5),
               dict(outs=(odd(4),) + (P,) * 8), dict(outs=(None,) + (P,) * 8), dict(back=np.array([0, -2, 0], np.int32))):
        assert forward(L.sushi_hip_track_forward_ordered_keep, **kw) == forward(L.sushi_hip_track_forward_ordered, **kw) != 0, kw


class _NoDevice(object):
    """A stream that fails the moment a search asks it for device memory: every check in front of that is host work."""
    sample_rate = 12000
    data = np.zeros((1, 12000 * 30), np.float32)

    def device_stream(self):
        return None

    def _pattern_source(self, patterns, dst_dev):
        return None, [0] * len(patterns), [p.shape[1] for p in patterns], True

    def _get_sample_for_time(self, t):
        return int(self.sample_rate * t) + 120000


def test_find_ordered_track_refuses_on_the_host():
    stream = _NoDevice()
    patterns = [np.zeros((1, 6000), np.uint8)] * 4
    centres = [1.0, 2.0, 3.0, 4.0]
    plain = 4 * 24001 * 6 + 3 * 24001 * 8
    kept = 4 * 24001 * 14 + 4 * 24001 * 8
    assert track.TrackState.nbytes(4, 24001, ordered=True) == plain
    assert track.TrackState.nbytes(4, 24001, ordered=True, margins=True) == kept
    assert track.TrackState.nbytes(4, 24001, ordered=True, margins=True, marginals=True) == kept + 4 * 24001 * 8
    for need, kw in ((kept, dict()), (kept + 4 * 24001 * 8, dict(marginals=True))):
        with pytest.raises(SushiError) as e:
            track.find_ordered_track(stream, patterns, centres, 1.0, 0.5, order=True, reach=4, margins=True, max_state_bytes=need - 1, **kw)
        assert str(need) in str(e.value) and str(need - 1) in str(e.value) and "max_state_bytes" in str(e.value)
        assert "4 events" in str(e.value) and "24001" in str(e.value) and str(plain) in str(e.value)
    with pytest.raises(SushiError) as e:
        track.find_ordered_track(stream, patterns, centres, 1.0, 0.5, order=True, reach=4, max_state_bytes=plain - 1)
    assert str(plain) in str(e.value) and "find_ordered_track" in str(e.value)
    for kw in (dict(guard=5), dict(marginals=True)):                               # they belong to margins=True
        with pytest.raises(SushiError) as e:
            track.find_ordered_track(stream, patterns, centres, 1.0, 0.5, reach=4, **kw)
        assert "margins=True" in str(e.value)
    for bad in ([1, 2, 3], [1] * 5, -1, "wide"):
        with pytest.raises(SushiError):
            track.find_ordered_track(stream, patterns, centres, 1.0, 0.5, reach=4, margins=True, guard=bad)
    for bad in (dict(order=[0, 0, 0]), dict(order=[None, 0, -2, 0]), dict(order="yes"), dict(penalty=[0.5, 0.5, 0.5]),
                dict(penalty=[0.0, 0.5, -0.5, 0.5]), dict(penalty=[0.0, 0.5, float("nan"), 0.5])):
        args = dict(penalty=0.5, reach=0, margins=True)
        args.update(bad)
        with pytest.raises(SushiError):
            track.find_ordered_track(stream, patterns, centres, 1.0, **args)
    with pytest.raises(SushiError) as e:
        track.find_ordered_track(stream, patterns, [1.0, 3.0, 2.0, 4.0], 1.0, 0.5, order=True, reach=0, margins=True)
    assert "event 2" in str(e.value)
    for bad in (dict(), dict(reach=1, max_rate=1e-3)):                             # exactly one of max_rate and reach
        with pytest.raises(SushiError):
            track.find_ordered_track(stream, patterns, centres, 1.0, 0.5, **bad)
    with pytest.raises(SushiError):
        track.find_ordered_track(stream, patterns, centres[:3], 1.0, 0.5, reach=1)
    # the two refusals of before stand
    with pytest.raises(SushiError):
        track.TrackState(3, 8, None, keep=True, ordered=True)
    with pytest.raises(SushiError):
        track.TrackState(3, 8, None, margins=True)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, reach=0, order=True, margins=True)
    assert "not built" in str(e.value)


def test_find_ordered_track_without_margins_is_find_track_with_order(monkeypatch):
    """Both entries hand the ordered search the same arguments: with margins=False find_ordered_track is find_track(order=...)."""
    seen = []
    monkeypatch.setattr(track, "_search", lambda *a, **kw: seen.append((a, kw)) or "found")
    stream, patterns, centres = object(), [np.zeros((1, 10), np.uint8)] * 3, [1.0, 2.0, 3.0]
    for order, penalty in ((True, 0.5), ([None, 3, 4], 0.5), (None, [0.0, 0.5, 0.25]), (True, [0.0, 0.5, 0.25])):
        del seen[:]
        kw = dict(reach=2, step_cost=0.01, slack=2, weights="length", method="ccoeff_normed", max_bytes=1 << 20, max_state_bytes=1 << 21,
                  clamp=0.5, capacity=7)
        assert track.find_track(stream, patterns, centres, 1.0, penalty, order=order, **kw) == "found"
        assert track.find_ordered_track(stream, patterns, centres, 1.0, penalty, order=order, **kw) == "found"
        (a, akw), (b, bkw) = seen
        # _search(name, ordered, wide, stream, ..., margins, guard, marginals, clamp, capacity): all but the name
        assert a[1:] == b[1:] and akw == bkw == {} and (a[0], b[0]) == ("find_track", "find_ordered_track")
        assert a[1:4] == (True, False, stream) and a[17:20] == (False, None, False) and len(a) == 22


# ---------------------------------------------------------------------------------------------- the scenario on the oracle
def test_the_decoy_scenario_has_its_recorded_ordered_margins(oracle):
    dst, src = ocases.streams()
    patterns, _centres, bases = ocases.scenario(dst, src)
    lens = [p.shape[1] for p in patterns]
    k_lo, n_shift = joint.joint_window(bases, lens, dst.data.shape[1], int(ocases.RATE * ocases.WINDOW))
    assert (k_lo, n_shift) == (ocases.K_LO, ocases.N_SHIFT)
    rows = ocases.oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift)
    back = track.order_back(bases, lens)
    got = track.track_ordered_margins_host(rows, [1.0] * 10, ocases.PENALTY, 0.0, 0, back, cases.GUARD)
    assert (got.shifts + k_lo).tolist() == ocases.TRUE_K and got.cost == cases.COST
    lams = [0.0] + [ocases.PENALTY] * 9
    S = _path_terms(got, rows, [1.0] * 10, lams, 0.0)
    assert (np.abs(got.through - got.cost) <= 6 * 10 * 2.0 ** -53 * S).all()
    margin = got.alt - got.through
    alt_k = (got.alt_arg + k_lo).tolist()
    assert (margin >= 0).all() and (got.best_arg + k_lo).tolist() == ocases.TRUE_K
    assert alt_k[2] == ocases.TRUE_K[2] + ocases.DECOYS[0] and alt_k[7] == ocases.TRUE_K[7] + ocases.DECOYS[1]     # the victims' decoys
    assert got.through.tolist() == cases.THROUGH and got.alt.tolist() == cases.ALT
    assert margin.tolist() == cases.MARGINS and alt_k == cases.ALT_K
    # the plain pass at this penalty follows the decoys: its margins are about another path
    plain = track.track_margins_host(rows, [1.0] * 10, ocases.PENALTY, 0.0, 0, cases.GUARD)
    assert (plain.shifts + k_lo).tolist() == ocases.RESULTS[ocases.PENALTY][0] != ocases.TRUE_K
