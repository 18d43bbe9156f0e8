"""Margins without a GPU: the NumPy restatement of sushi_hip_track_margins (sushi_amd/track.py track_margins_host) against a brute
force over all paths, its three stated facts (the exact path minimum, the reversal identity, consistency with the total), the guard
window's edges, the kernels' own header compiled for the CPU (tests/host_track_margins_check.cpp, a program of its own under
AddressSanitizer + UBSan), the entry points' argument checks, and the two scenarios: two explanations planted, and the wandering
shift on the CPU oracle."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import track_cases as cases
import track_margin_cases as mcases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, joint, track
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP = -32768


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("track_margins_check")), "host_track_margins_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_track_margins_check.cpp"), "-o", exe])
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


def _cheapest(c, a, b, r, lam, mu):
    """What the step between shifts a and b adds to c: the cheaper allowed choice of a move's price (nothing for a == b) and lam."""
    d = abs(a - b)
    choices = [c + lam]
    if d == 0:
        choices.append(c)
    elif d <= r:
        choices.append(c + mu * float(d))
    return min(choices)


def _through_path(rows, weights, lam, mu, reach, method, path, e):
    """(prefix cost of events 0 .. e, accumulated forwards) + (suffix cost of events E-1 .. e+1, accumulated backwards, and the step
    into it from event e; u_e is not added again)."""
    E = len(rows)
    p = _u(rows, weights, method, 0, path[0])
    for i in range(1, e + 1):
        p = _u(rows, weights, method, i, path[i]) + _cheapest(p, path[i - 1], path[i], reach[i], lam, mu)
    if e == E - 1:
        return p
    c = _u(rows, weights, method, E - 1, path[E - 1])
    for i in range(E - 2, e, -1):
        c = _u(rows, weights, method, i, path[i]) + _cheapest(c, path[i], path[i + 1], reach[i + 1], lam, mu)
    return p + _cheapest(c, path[e], path[e + 1], reach[e + 1], lam, mu)


@pytest.mark.parametrize("method", METHODS)
def test_every_marginal_is_the_minimum_over_all_paths_through_it(method):
    """E <= 4 rows over n <= 7 shifts, random float32 rows and dyadic ones with planted ties, reaches 0 .. 3, weights including 0:
    every M_e[j] is bitwise the minimum over all n^E paths with s_e = j; through, best and alt are NumPy's on those rows."""
    rng = np.random.default_rng(11)
    sign = -1.0 if method == "ccoeff_normed" else 1.0
    seen_alt = seen_none = False
    for trial, (E, n) in enumerate([(1, 1), (1, 5), (2, 3), (2, 7), (3, 5), (3, 6), (4, 4), (4, 7), (4, 7)]):
        if trial % 2:       # dyadic values: every sum exact, ties are real ties (never 0: a weighted cost keeps its sign)
            rows = [(sign * rng.integers(1, 9, n) / 8.0).astype(np.float32) for _ in range(E)]
            lam, mu = (0.25, 0.125, 0.5, 1.0)[trial % 4], (0.0, 0.125, 0.25)[trial % 3]
        else:
            rows = [(sign * (rng.random(n, dtype=np.float32) * np.float32(0.875) + np.float32(0.0625))).astype(np.float32) for _ in range(E)]
            lam, mu = (0.3, 1.0 / 3.0, 0.05)[trial % 3], (1e-2, 0.0, 0.07)[trial % 3]
        weights = [(1.0, 0.0, 2.5, 1.0 / 3.0)[(e + trial) % 4] for e in range(E)]
        weights[0] = weights[0] or 1.0
        reach = [int(k) for k in rng.integers(0, 4, E)]
        guard = [int(k) for k in rng.integers(0, n + 1, E)]
        got = track.track_margins_host(rows, weights, lam, mu, reach, guard, method)
        reach[0] = 0
        paths = list(itertools.product(range(n), repeat=E))
        for e in range(E):
            costs = [_through_path(rows, weights, lam, mu, reach, method, p, e) for p in paths]
            for j in range(n):
                want = min(c for c, p in zip(costs, paths) if p[e] == j)
                assert _bits64(got.marginals[e, j]) == _bits64(want), (E, n, e, j)
        _np_reductions(got, guard)
        assert (_bits64(got.marginals[E - 1]) == _bits64(got.D[E - 1])).all()
        plain = track.track_host(rows, weights, lam, mu, reach, method)
        assert plain.shifts.tolist() == got.shifts.tolist() and _bits64(plain.cost) == _bits64(got.cost)
        assert (plain.moves == got.moves).all() and (_bits64(got.D[:, :].min(axis=1)) == _bits64(got.row_min)).all()
        seen_alt |= bool((got.alt_arg >= 0).any())
        seen_none |= bool((got.alt_arg < 0).any())
    assert seen_alt and seen_none


# ---------------------------------------------------------------------------------------------- the three facts, synthetic sequences
@pytest.fixture(scope="module", params=METHODS)
def sequences(request):
    out = {}
    for E, n, reach in cases.SHAPES:
        curves, rows, weights, lam, rs, mu = cases.sequence(E, n, reach, request.param, seed=3)
        guard = mcases.guards(E, n)
        out[(E, n, reach)] = (cases.rows_of(curves, rows, n), weights, lam, rs, mu, guard,
                              track.track_margins_host(cases.rows_of(curves, rows, n), weights, lam, mu, rs, guard, request.param))
    return request.param, out


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_the_three_facts(sequences, shape):
    method, table = sequences
    rows, weights, lam, rs, mu, guard, got = table[shape]
    E, n = shape[0], shape[1]
    # reversal: n_0 is the tracking pass's total of the reversed sequence, reach_rev[i] = reach[E - i]
    rev = track.track_host(rows[::-1], weights[::-1], lam, mu, [0] + [rs[E - i] for i in range(1, E)], method)
    assert _bits64(rev.cost) == _bits64(got.c_min[0])
    assert (_bits64(rev.row_min[::-1]) == _bits64(got.c_min)).all()
    # consistency: best <= through and best <= alt exactly; through is the total up to summation order
    assert (got.best <= got.through).all() and (got.best <= got.alt).all()
    S = mcases.path_terms(got, rows, weights, lam, mu, method)
    assert (np.abs(got.through - got.cost) <= 6 * E * 2.0 ** -53 * S).all(), (np.abs(got.through - got.cost).max(), S)
    assert all(_bits64(got.marginals[e, got.best_arg[e]]) == _bits64(got.best[e]) for e in range(E))
    _np_reductions(got, guard)


def test_all_reach_zero_is_the_same_statement_about_the_segmentation_model():
    from sushi_amd import segments
    rows = [r for r in cases.rows_of(*cases.sequence(7, 64, 3, "sqdiff_normed", seed=3)[:2], 64)]
    weights = [1.0, 1.0 / 3.0, 0.0, 2.5, 1.0, 1.0 / 3.0, 0.0]
    got = track.track_margins_host(rows, weights, 0.0625, 0.5, 0, 1)
    want = segments.path_host(rows, weights, 0.0625)
    assert got.shifts.tolist() == want.shifts.tolist() and _bits64(got.cost) == _bits64(want.cost)
    assert (got.best <= got.through).all()


# ---------------------------------------------------------------------------------------------- the guard window
def test_guard_edges():
    lone = np.array([0.5, 0.25, 0.9, 0.1, 0.9, 0.25, 0.5], np.float32)
    one = lambda g: track.track_margins_host([lone], [1.0], 0.5, 0.0, 0, g)
    # E = 1: M is u itself.  s = 3; equal values on both sides of the window: the first index
    got = one(1)
    assert got.shifts.tolist() == [3] and (_bits64(got.marginals[0]) == _bits64(lone.astype(np.float64))).all()
    assert (got.alt_arg.tolist(), got.alt.tolist(), got.best_arg.tolist()) == ([1], [0.25], [3])
    assert _bits64(got.through[0]) == _bits64(np.float64(np.float32(0.1))) == _bits64(got.c_min[0])
    got = one(0)                                        # guard 0: only s itself is left out; 0.25 at 1 before 0.25 at 5
    assert got.alt_arg.tolist() == [1]
    got = one(2)                                        # the window covers 1 .. 5: 0.5 at 0 before 0.5 at 6
    assert (got.alt_arg.tolist(), got.alt.tolist()) == ([0], [0.5])
    got = one(3)                                        # the window ends exactly at both axis ends: nothing outside
    assert got.alt_arg.tolist() == [-1] and got.alt.tolist() == [np.inf]
    for g in (7, 8, 2 ** 31 - 1):                       # guard >= n_shift
        got = one(g)
        assert got.alt_arg.tolist() == [-1] and got.alt.tolist() == [np.inf] and got.best_arg.tolist() == [3]
    # s at 0 and at n - 1; a window that ends exactly at the axis end on the other side
    first = np.array([0.1, 0.9, 0.3, 0.9, 0.2], np.float32)
    got = track.track_margins_host([first], [1.0], 0.5, 0.0, 0, 3)
    assert got.shifts.tolist() == [0] and got.alt_arg.tolist() == [4] and got.alt.tolist() == [float(np.float32(0.2))]
    assert track.track_margins_host([first], [1.0], 0.5, 0.0, 0, 4).alt_arg.tolist() == [-1]
    assert track.track_margins_host([first], [1.0], 0.5, 0.0, 0, 1).alt_arg.tolist() == [4]
    got = track.track_margins_host([first[::-1].copy()], [1.0], 0.5, 0.0, 0, 3)
    assert got.shifts.tolist() == [4] and got.alt_arg.tolist() == [0]
    assert track.track_margins_host([first[::-1].copy()], [1.0], 0.5, 0.0, 0, 4).alt_arg.tolist() == [-1]
    # one guard per row
    got = track.track_margins_host([lone, lone], [1.0, 1.0], 0.5, 0.0, 0, [0, 3])
    assert got.alt_arg.tolist() == [1, -1] and got.shifts.tolist() == [3, 3]
    for bad in (-1, [1], [1, 2, 3], "wide", [0, None], 2 ** 31):
        with pytest.raises(SushiError):
            track.track_margins_host([lone, lone], [1.0, 1.0], 0.5, 0.0, 0, bad)
    with pytest.raises(SushiError) as e:
        track.checked_guard([0, 5, -2], 3, first_row=4)
    assert "event 6" in str(e.value) and "-2" in str(e.value)
    assert track.checked_guard(7, 3).tolist() == [7, 7, 7] and track.checked_guard(7, 3).dtype == np.int32


# ---------------------------------------------------------------------------------------------- two explanations, planted
def test_a_run_with_two_explanations_has_small_margins_and_an_anchor_raises_them():
    lam, mu, reach, guard = mcases.TWO_PENALTY, mcases.TWO_STEP_COST, mcases.TWO_REACH, mcases.TWO_GUARD
    got = track.track_margins_host(mcases.two_explanations(), [1.0] * 6, lam, mu, reach, guard)
    margin = got.alt - got.through
    assert got.shifts.tolist() == [100] * 6 and got.alt_arg.tolist() == [300] * 6
    assert np.abs(margin - 0.12).max() < 1e-6 and (margin < lam).all()         # no anchor: the margins say so
    got = track.track_margins_host(mcases.two_explanations(anchor=2), [1.0] * 6, lam, mu, reach, guard)
    margin = got.alt - got.through
    assert got.shifts.tolist() == [100] * 6 and got.alt_arg.tolist() == [300] * 6
    assert np.abs(margin - np.array([0.32, 0.34, 0.90, 0.36, 0.34, 0.32])).max() < 1e-6 and (margin > lam).all()
    # event 2 alone at 300 would cost 0.8 + 2 * 0.3 = 1.40: the margin counts that its neighbours come along
    assert margin[2] < 1.40 - 0.4


# ---------------------------------------------------------------------------------------------- the kernels' header on the CPU
EXPECTED_RC = {   # case of host_track_margins_check validate -> what stage_margins returns
    "good": 0, "good_ccoeff": 0, "null_rows": -1, "null_reach": -1, "null_guard": -1, "null_mem": -1, "method_2": -1, "no_rows": -1,
    "no_shift": -1, "empty_curves": -1, "shift_beyond_curves": -1, "whole_sequence": 0, "rows_end_at_sequence_end": 0,
    "rows_past_sequence_end": -1, "row0_negative": -1, "row0_at_end": -1, "no_total": -1, "rows_end_at_int_max": 0,
    "rows_sum_overflows_int": -1, "row_before_curves": -1, "row_ends_at_curves_end": 0, "row_one_past_curves_end": -1,
    "row_sum_overflows": -1, "weight_nan": -1, "weight_negative": -1, "penalty_nan": -1, "penalty_negative": -1, "step_cost_inf": -1,
    "step_cost_negative": -1, "reach_of_the_calls_first_row_is_ignored": 0, "reach_1025": -1, "reach_negative": -1,
    "reach_of_the_row_after_the_call": -1, "negative_reach_of_the_row_after_the_call": -1,
    "no_row_after_the_call_its_entry_is_not_read": 0, "reach_all_widest": 0, "guard_negative": -1, "guard_int_min": -1, "guard_zero": 0,
    "workspace_exact": 0, "workspace_short": -4, "workspace_none": -4, "workspace_misaligned": -2,
    "workspace_misaligned_and_short": -2, "bad_guard_before_workspace": -1, "bad_reach_before_alignment": -1}


def test_stage_margins_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = dict(l.split() for l in lines[:len(EXPECTED_RC)])
    assert {k: int(v) for k, v in got.items()} == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    # two sets of one record of 36 bytes per workgroup (three float64 minima and their int32 indices), each set padded to 256 bytes
    assert rest[0] == "bytes 512 512 %d %d 0 0 0" % (2 * 16896, 2 * 73728)
    # |j - s| > guard: s itself is inside at guard 0; no sum overflows at a guard of 2^31 - 1; 125 is inside 5 +- 120, 126 outside
    assert rest[1] == "outside 0 1 1 0 0 0 1"
    assert rest[2] == "facts_one rc=0 per=2 items=1 grid=1 first=1 set=256 bytes=512 offsets=(0,8,16,24,28,32)"
    assert rest[3] == "facts_513 rc=0 per=2 items=2 grid=2 first=1 set=256 bytes=512 offsets=(0,16,32,48,56,64)"
    assert rest[4] == "facts_240001 rc=0 per=2 items=469 grid=469 first=1 set=16896 bytes=33792 offsets=(0,3752,7504,11256,13132,15008)"
    assert rest[5].startswith("facts_int32_max rc=0 per=8 items=1048576 grid=2048 first=1 set=73728 bytes=147456 ")
    assert len(rest) == 6


def _run_check(check, tmp_path, method, lam, mu, n, curves, rows, reach, guard):
    rt = np.array(rows, dtype=_native.JOINT_ROW_DTYPE)
    paths = [os.path.join(str(tmp_path), name) for name in ("curves", "rows", "reach", "guard", "out")]
    curves.tofile(paths[0])
    rt.tofile(paths[1])
    np.array(reach, np.int32).tofile(paths[2])
    np.array(guard, np.int32).tofile(paths[3])
    subprocess.check_call([check, "pass", method.split("_")[0], float(lam).hex(), float(mu).hex(), str(n)] + paths)
    raw = np.fromfile(paths[4], np.uint8)
    E = len(rows)
    through, best, alt, c_min = (raw[8 * E * k:8 * E * (k + 1)].view(np.uint64) for k in range(4))
    best_arg, alt_arg, shifts = (raw[32 * E + 4 * E * k:32 * E + 4 * E * (k + 1)].view(np.int32) for k in range(3))
    M, D = (raw[44 * E + 8 * E * n * k:44 * E + 8 * E * n * (k + 1)].view(np.uint64).reshape(E, n) for k in range(2))
    return through, best, alt, c_min, best_arg, alt_arg, shifts, M, D


def _compare_with_host(got, want):
    through, best, alt, c_min, best_arg, alt_arg, shifts, M, D = got
    assert shifts.tolist() == want.shifts.tolist()
    assert (D == _bits64(want.D)).all() and (M == _bits64(want.marginals)).all()
    assert (through == _bits64(want.through)).all() and (best == _bits64(want.best)).all() and (alt == _bits64(want.alt)).all()
    assert (c_min == _bits64(want.c_min)).all()
    assert best_arg.tolist() == want.best_arg.tolist() and alt_arg.tolist() == want.alt_arg.tolist()


@pytest.mark.parametrize("method", METHODS)
def test_the_header_on_the_cpu_equals_track_margins_host(check, tmp_path, method):
    """margin_back, margin_through, margin_suffix, margin_outside, the candidates of track_core.hpp and the first-minimum rule, run
    by a program of its own over the sequences of the GPU test but the longest -- divided as the kernels divide them, every open
    order taken backwards, the sequence walked in two calls."""
    for E, n, reach in cases.SHAPES[:-1] + [(4, 1025, 600), (3, 5, 1024), (4, 7, 64)]:
        curves, rows, weights, lam, rs, mu = cases.sequence(E, n, reach, method, seed=3)
        guard = mcases.guards(E, n)
        want = track.track_margins_host(cases.rows_of(curves, rows, n), weights, lam, mu, rs, guard, method)
        _compare_with_host(_run_check(check, tmp_path, method, lam, mu, n, curves, rows, rs, guard), want)
    for centre in (511, 512):
        a, b = cases.tie_rows(1024, centre, method)
        curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b])
        for guard in ([1, 1], [0, 600]):
            want = track.track_margins_host([a, b], [1.0, 1.0], 0.5, 0.0, [0, 3], guard, method)
            _compare_with_host(_run_check(check, tmp_path, method, 0.5, 0.0, 1024, curves, [(1, 1.0), (1027, 1.0)], [0, 3], guard), want)


# ---------------------------------------------------------------------------------------------- the entry points, no GPU
def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    assert {"sushi_hip_track_forward_keep", "sushi_hip_track_margins_bytes", "sushi_hip_track_margins"} <= set(_native.declared_symbols())
    assert L.sushi_hip_track_margins_bytes(1, 1) == 512 and L.sushi_hip_track_margins_bytes(200, 240001) == 33792
    assert L.sushi_hip_track_margins_bytes(0, 5) == 0 and L.sushi_hip_track_margins_bytes(5, 0) == 0
    rows = np.array([(0, 1.0), (501, 0.0), (333, 2.5)], dtype=_native.JOINT_ROW_DTYPE)
    reach = np.array([9999, 1024, 17, 3], np.int32)
    guard = np.array([0, 120, 2 ** 31 - 1], np.int32)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)
    EINVAL, EALIGN = -1, -2

    def call(curves=P, n_curve=1000, rows=rows, reach=reach, guard=guard, n_rows=3, n_shift=499, method=0, penalty=0.5, step_cost=1e-3,
             row0=2, n_total=7, ptrs=(P,) * 9, M=None, mem=P, mem_bytes=1 << 16):
        return L.sushi_hip_track_margins(curves, n_curve, None if rows is None else rows.ctypes.data,
                                         None if reach is None else reach.ctypes.data, None if guard is None else guard.ctypes.data,
                                         n_rows, n_shift, method, penalty, step_cost, row0, n_total, *ptrs, M, mem, mem_bytes, None)

    assert call(curves=None) == EINVAL and call(rows=None) == EINVAL and call(reach=None) == EINVAL and call(guard=None) == EINVAL
    assert call(mem=None) == EINVAL
    for k in range(9):
        assert call(ptrs=tuple(None if i == k else P for i in range(9))) == EINVAL, k
    assert call(method=2) == EINVAL and call(n_rows=0) == EINVAL and call(n_shift=0) == EINVAL and call(n_shift=1001) == EINVAL
    assert call(row0=-1) == EINVAL and call(row0=5) == EINVAL and call(n_total=0) == EINVAL
    assert call(row0=2 ** 31 - 3, n_total=2 ** 31 - 1) == EINVAL          # row0 + n_rows would pass int: never formed
    for bad in (np.nan, np.inf, -1e-300):
        assert call(penalty=bad) == EINVAL and call(step_cost=bad) == EINVAL
    for at, value, rc in ((0, -7, _native.ENOSPACE), (1, 1025, EINVAL), (2, -1, EINVAL), (3, 1025, EINVAL)):
        r = reach.copy()
        r[at] = value
        assert call(reach=r, mem_bytes=16) == rc, (at, value)
    for at in range(3):
        g = guard.copy()
        g[at] = -1
        assert call(guard=g) == EINVAL
    # every check passes up to the workspace, M_dev null or not
    assert call(mem_bytes=16) == _native.ENOSPACE and call(mem_bytes=16, M=P) == _native.ENOSPACE and call(mem=odd(128)) == EALIGN
    assert call(curves=odd(2)) == EALIGN and call(M=odd(4)) == EALIGN
    for k, off in enumerate((4, 2, 4, 4, 4, 4, 2, 4, 2)):   # D_all, shift, C, c_min, through, best, best_arg, alt, alt_arg
        assert call(ptrs=tuple(odd(off) if i == k else P for i in range(9))) == EALIGN, k
    # forward_keep: sushi_hip_track_forward's refusals
    steps = np.array([5, 1024, 17], np.int32)
    fwd = lambda **kw: L.sushi_hip_track_forward_keep(P, 1000, rows.ctypes.data, steps.ctypes.data, 3, kw.get("n_shift", 499), 0, 0.5, 1e-3,
                                                      kw.get("row0", 2), 7, kw.get("D", P), P, P, P, P, P, P, kw.get("mem_bytes", 16), None)
    assert fwd() == _native.ENOSPACE and fwd(n_shift=0) == EINVAL and fwd(row0=5) == EINVAL and fwd(D=None) == EINVAL
    assert fwd(D=odd(4), mem_bytes=1 << 16) == EALIGN


class _NoDevice(object):
    """A stream that fails the moment find_track asks it for device memory: every check in front of that is host work."""
    sample_rate = 12000
    data = np.zeros((1, 400000), np.uint8)

    def device_stream(self):
        return None

    def _pattern_source(self, patterns, dst_dev):
        return None, [0] * len(patterns), [p.shape[1] for p in patterns], True

    def _get_sample_for_time(self, t):
        return int(self.sample_rate * t) + 120000


def test_find_track_with_margins_refuses_on_the_host():
    stream = _NoDevice()
    patterns = [np.zeros((1, 6000), np.uint8)] * 4
    centres = [1.0, 2.0, 3.0, 4.0]
    plain = 4 * 24001 * 2 + 2 * 24001 * 8
    kept = 4 * 24001 * 2 + 4 * 24001 * 8 + 2 * 24001 * 8
    assert track.TrackState.nbytes(4, 24001) == plain and track.TrackState.nbytes(4, 24001, keep=True) == kept
    assert track.TrackState.nbytes(4, 24001, keep=True, marginals=True) == kept + 4 * 24001 * 8
    for need, kw in ((kept, dict()), (kept + 4 * 24001 * 8, dict(marginals=True))):
        with pytest.raises(SushiError) as e:
            track.find_track(stream, patterns, centres, 1.0, 0.5, reach=4, margins=True, max_state_bytes=need - 1, **kw)
        assert str(need) in str(e.value) and str(need - 1) in str(e.value) and "max_state_bytes" in str(e.value)
        assert "4 events" in str(e.value) and "24001" in str(e.value)
    for bad in ([1, 2, 3], [1] * 5, -1, "wide"):
        with pytest.raises(SushiError):
            track.find_track(stream, patterns, centres, 1.0, 0.5, reach=4, margins=True, guard=bad)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, reach=4, margins=True, guard=[1, 2, 3])
    assert "3 guards" in str(e.value) and "4 rows" in str(e.value)
    for kw in (dict(guard=5), dict(marginals=True)):                               # they belong to margins=True
        with pytest.raises(SushiError):
            track.find_track(stream, patterns, centres, 1.0, 0.5, reach=4, **kw)


# ---------------------------------------------------------------------------------------------- the scenario on the oracle
def test_the_wandering_shift_scenario_has_its_recorded_margins(oracle):
    dst, src = cases.streams()
    patterns, _centres, bases = cases.scenario(dst, src)
    k_lo, n_shift = joint.joint_window(bases, [p.shape[1] for p in patterns], dst.data.shape[1], int(cases.RATE * cases.WINDOW))
    assert (k_lo, n_shift) == (cases.K_LO, cases.N_SHIFT) == (-12000, 24001)
    rows = cases.oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift)
    got = track.track_margins_host(rows, [1.0] * 10, mcases.PENALTY, mcases.STEP_COST, cases.REACH, mcases.GUARD)
    assert (got.shifts + k_lo).tolist() == cases.TRUE_K and got.cost == mcases.COST
    S = mcases.path_terms(got, rows, [1.0] * 10, mcases.PENALTY, mcases.STEP_COST)
    assert (np.abs(got.through - got.cost) <= 6 * 10 * 2.0 ** -53 * S).all()
    margin = got.alt - got.through
    alt_k = (got.alt_arg + k_lo).tolist()
    assert alt_k[2] == cases.LONE_K[2] == -4125 and alt_k[7] == cases.LONE_K[7] == 3590       # the victims' decoys
    assert abs(margin[2] - 0.4420) < 1e-3 and abs(margin[7] - 0.4376) < 1e-3
    assert (margin > 0).all() and int(np.argmin(margin)) == 6 and abs(margin[6] - 0.2650) < 1e-3
    assert got.through.tolist() == mcases.THROUGH and got.alt.tolist() == mcases.ALT
    assert margin.tolist() == mcases.MARGINS and alt_k == mcases.ALT_K
    assert (got.best_arg + k_lo).tolist() == cases.TRUE_K
