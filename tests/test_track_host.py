"""Tracking without a GPU: the NumPy restatement of sushi_hip_track_forward / sushi_hip_track_backtrack (sushi_amd/track.py
track_host) against the recursion written out on Python floats and against a brute force over all paths, reach 0 against path_host,
planted ties, penalty extremes, the kernels' own header compiled for the CPU (tests/host_track_check.cpp, a program of its own under
AddressSanitizer + UBSan), the entry points' argument checks, and the wandering-shift scenario on the CPU oracle."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import track_cases as cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, joint, segments, track
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP = -32768


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("track_check")), "host_track_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_track_check.cpp"), "-o", exe])
    return exe


def _loop(rows, weights, lam, mu, reach, method):
    """The definition, written out: one shift and one candidate at a time on Python floats (IEEE float64), the candidates compared as
    (value, |d|, d > 0) tuples.  -> (shifts, cost, row_min, row_arg, moves)"""
    E, n = len(rows), rows[0].shape[0]
    D, moves, row_min, row_arg = None, [[0] * n], [], []
    for e in range(E):
        u = [float(weights[e]) * (-float(rows[e][j]) if method == "ccoeff_normed" else float(rows[e][j])) for j in range(n)]
        if e == 0:
            D = u
        else:
            jump = row_min[e - 1] + lam
            new, mv = [], []
            for j in range(n):
                cands = [(D[j], 0, False)]
                for d in range(-reach[e], reach[e] + 1):
                    if d != 0 and 0 <= j + d < n:
                        cands.append((D[j + d] + mu * float(abs(d)), abs(d), d > 0))
                near, ad, pos = min(cands)
                take = near <= jump
                new.append(u[j] + (near if take else jump))
                mv.append((ad if pos else -ad) if take else JUMP)
            D = new
            moves.append(mv)
        at = 0
        for j in range(1, n):
            if D[j] < D[at]:
                at = j
        row_arg.append(at)
        row_min.append(D[at])
    s = row_arg[-1]
    shifts = [s]
    for e in range(E - 1, 0, -1):
        s = row_arg[e - 1] if moves[e][s] == JUMP else s + moves[e][s]
        shifts.append(s)
    return shifts[::-1], row_min[-1], row_min, row_arg, moves


def _first(row, method):
    at = 0
    for j in range(1, row.shape[0]):
        if (row[j] > row[at]) if method == "ccoeff_normed" else (row[j] < row[at]):
            at = j
    return at


def _rows(E, n, seed, method="sqdiff_normed"):
    rng = np.random.default_rng(seed)
    lo = 0.0 if method == "sqdiff_normed" else -1.0
    return [(rng.random(n, dtype=np.float32) * np.float32(1.0 - lo) + np.float32(lo)).astype(np.float32) for _ in range(E)]


def _path_cost(rows, weights, lam, mu, reach, method, path):
    """A path's cost accumulated in the pass's order: c = u_0[s_0]; per event the cheaper allowed choice of c + mu |d| (a move within
    reach; c itself for d = 0) and c + lam (a jump), then c = u_e[s_e] + c."""
    u = lambda e: float(weights[e]) * (-float(rows[e][path[e]]) if method == "ccoeff_normed" else float(rows[e][path[e]]))
    c = u(0)
    for e in range(1, len(rows)):
        d = abs(path[e] - path[e - 1])
        choices = [c + lam]
        if d == 0:
            choices.append(c)
        elif d <= reach[e]:
            choices.append(c + mu * float(d))
        c = u(e) + min(choices)
    return c


# ---------------------------------------------------------------------------------------------- track_host
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("E", [1, 2, 7, 33])
@pytest.mark.parametrize("n", [1, 63, 65, 1025])
def test_track_host_is_the_recursion_written_out(E, n, method):
    for reach in (0, 1, 3, 64):
        rows = _rows(E, n, seed=E * 10007 + n + reach, method=method)
        rs = [reach] * E if reach < 2 else cases.reaches(E, reach)
        weights, lam, mu = (([1.0] * E, 0.25, 2.0 ** -7), ([(1.0 / 3.0, 0.0, 2.5)[i % 3] for i in range(E)], 1.0 / 3.0, 1e-3),
                            ([1.0] * E, 0.125, 0.0), ([1.0] * E, 0.0, 0.01))[(reach + E) % 4]
        got = track.track_host(rows, weights, lam, mu, rs, method)
        shifts, cost, row_min, row_arg, moves = _loop(rows, weights, lam, mu, [0] + list(rs[1:]), method)
        assert got.shifts.tolist() == shifts and got.row_arg.tolist() == row_arg, (reach,)
        assert (_bits64(got.row_min) == _bits64(row_min)).all() and _bits64(got.cost) == _bits64(cost)
        assert got.moves.tolist() == moves
        own = [_first(r, method) for r in rows]
        assert got.row_own_index.tolist() == own
        assert (_bits(got.row_own_scores) == _bits([r[k] for r, k in zip(rows, own)])).all()
        assert got.shifts.dtype == np.int32 and got.moves.dtype == np.int16 and got.row_min.dtype == np.float64
        assert got.moves.shape == (E, n)


@pytest.mark.parametrize("method", METHODS)
def test_the_pass_finds_the_minimum_over_all_paths(method):
    """E <= 5, n_shift <= 4, reach <= 2, dyadic values (every sum exact, so ties are real ties): track_host's cost is the minimum
    over all n_shift^E paths of the in-order cost, exactly, and its own path attains it."""
    rng = np.random.default_rng(6)
    sign = -1.0 if method == "ccoeff_normed" else 1.0
    seen_move = seen_jump = False
    for E, n in itertools.product((1, 2, 3, 5), (1, 2, 3, 4)):
        for trial in range(8):
            rows = [(sign * rng.integers(0, 17, n) / 16.0).astype(np.float32) for _ in range(E)]
            weights = [(1.0, 0.5, 2.0, 0.0)[int(k)] for k in rng.integers(0, 4, E)]
            lam = (0.0, 0.125, 0.5, 1.0, 4.0, 0.3, 0.25, 2.0)[trial]
            mu = (0.0, 0.0625, 0.25, 0.125, 1.0, 0.1, 0.0, 0.5)[(trial + E) % 8]
            reach = [int(k) for k in rng.integers(0, 3, E)]
            got = track.track_host(rows, weights, lam, mu, reach, method)
            reach[0] = 0
            costs = [_path_cost(rows, weights, lam, mu, reach, method, p) for p in itertools.product(range(n), repeat=E)]
            assert got.cost == min(costs), (E, n, trial)
            assert _path_cost(rows, weights, lam, mu, reach, method, got.shifts.tolist()) == got.cost, (E, n, trial)
            words = [int(got.moves[e, got.shifts[e]]) for e in range(1, E)]
            seen_move |= any(w not in (0, JUMP) for w in words)
            seen_jump |= JUMP in words
    assert seen_move and seen_jump


@pytest.mark.parametrize("method", METHODS)
def test_all_reach_zero_is_path_host(method):
    for E, n in ((1, 1), (2, 63), (7, 65), (33, 1025)):
        rows = _rows(E, n, seed=E + n, method=method)
        weights = [(1.0, 1.0 / 3.0, 0.0, 2.5)[i % 4] for i in range(E)]
        for lam in (0.0, 0.0625, 1.0):
            want = segments.path_host(rows, weights, lam, method)
            for mu in (0.0, 0.5):
                got = track.track_host(rows, weights, lam, mu, 0, method)
                assert got.shifts.tolist() == want.shifts.tolist() and got.row_arg.tolist() == want.row_arg.tolist()
                assert (_bits64(got.row_min) == _bits64(want.row_min)).all() and _bits64(got.cost) == _bits64(want.cost)
                assert got.row_own_index.tolist() == want.row_own_index.tolist()
                assert (_bits(got.row_own_scores) == _bits(want.row_own_scores)).all()
                # a move word is 0 exactly where the path pass's stay bit is set
                stay = cases.segment_cases.stay_words(rows, weights, lam, method)
                for e in range(1, E):
                    bits = [(int(stay[e, j >> 6]) >> (j & 63)) & 1 for j in range(n)]
                    assert [int(m == 0) for m in got.moves[e]] == bits and set(got.moves[e].tolist()) <= {0, JUMP}


def test_equal_candidates_on_both_sides_take_the_negative_move():
    # D_0 = [0.25, 0.75, 0.25]: at j = 1, cand(-1) == cand(+1) == 0.25 + mu: -1 wins; and with a wider reach the smaller |d| wins
    a = np.array([0.25, 0.75, 0.25], np.float32)
    got = track.track_host([a, np.zeros(3, np.float32)], [1.0, 1.0], 1.0, 0.125, 1)
    assert got.moves[1].tolist() == [0, -1, 0] and got.row_min.tolist() == [0.25, 0.25] and got.shifts.tolist() == [0, 0]
    b = np.array([0.25, 0.25, 0.75, 0.25, 0.25], np.float32)
    got = track.track_host([b, np.zeros(5, np.float32)], [1.0, 1.0], 1.0, 0.0, 2)
    assert got.moves[1].tolist() == [0, 0, -1, 0, 0]
    for centre in (511, 512):
        rows = cases.tie_rows(1024, centre, "sqdiff_normed")
        got = track.track_host(rows, [1.0, 1.0], 0.5, 0.0, 3)
        assert got.moves[1, centre] == -1 and got.moves[1, 0] == 0 and got.moves[1, 1023] == 0
        assert got.moves[1, centre - 2] == 1 and got.moves[1, centre + 2] == -1


def test_a_free_move_does_not_beat_staying():
    # mu = 0: cand(0) == cand(+-1) wherever neighbours are equal: 0 wins
    got = track.track_host([np.array([0.5, 0.5, 0.5, 0.5], np.float32)] * 3, [1.0] * 3, 0.25, 0.0, 1)
    assert got.moves[1:].tolist() == [[0] * 4] * 2 and got.shifts.tolist() == [0, 0, 0] and got.cost == 1.5


def test_a_tie_between_moving_and_jumping_moves():
    # D_0 = [0.25, 0.5, 1.0], mu = 0.25, lam = 0.5: at j = 2, near = 0.5 + 0.25 = jump = 0.25 + 0.5: the tie moves, by -1
    rows = [np.array([0.25, 0.5, 1.0], np.float32), np.array([0.75, 0.75, 0.0], np.float32)]
    got = track.track_host(rows, [1.0, 1.0], 0.5, 0.25, 1)
    # (at j = 1, cand(0) = 0.5 == cand(-1) = 0.25 + 0.25: the smaller |d| wins)
    assert got.moves[1].tolist() == [0, 0, -1] and got.shifts.tolist() == [1, 2] and got.row_min.tolist() == [0.25, 0.75]
    assert got.row_arg.tolist() == [0, 2]
    rows[1] = np.array([0.75, 0.75, -0.25], np.float32)
    got = track.track_host(rows, [1.0, 1.0], 0.5, 0.25, 1)
    assert got.shifts.tolist() == [1, 2] and got.cost == 0.5 and got.moves[1, 2] == -1
    # one ulp above the tie jumps
    rows[0] = np.array([0.25, np.nextafter(np.float32(0.5), np.float32(1.0)), 1.0], np.float32)
    got = track.track_host(rows, [1.0, 1.0], 0.5, 0.25, 1)
    assert got.moves[1, 2] == JUMP and got.shifts.tolist() == [0, 2] and got.cost == 0.5


def test_negative_zero_passes_through_a_stay_under_ccoeff():
    """cand(0) is the value itself: D_0[1] = 1.0 * -(0.0) = -0.0 keeps its sign through row 1, whose u is -0.0 as well; a moved
    candidate has a price added (-0.0 + 0.0 = 0.0).  0.0 and -0.0 tie: the first index is the minimum."""
    a = np.array([-0.5, 0.0, -0.0, 0.0], np.float32)
    b = np.array([-0.5, 0.0, 0.0, 0.0], np.float32)
    got = track.track_host([a, b], [1.0, 1.0], 0.5, 0.0, 1, "ccoeff_normed")
    assert got.row_arg.tolist() == [1, 1] and got.shifts.tolist() == [1, 1] and got.moves[1].tolist() == [1, 0, 0, 0]
    assert _bits64(got.row_min).tolist() == [1 << 63, 1 << 63]
    shifts, cost, row_min, row_arg, moves = _loop([a, b], [1.0, 1.0], 0.5, 0.0, [0, 1], "ccoeff_normed")
    assert (shifts, row_arg) == ([1, 1], [1, 1]) and _bits64(row_min).tolist() == [1 << 63, 1 << 63]
    assert _bits(got.row_own_scores).tolist() == [0x00000000, 0x00000000] and got.row_own_index.tolist() == [1, 1]


def test_a_row_of_weight_zero_follows_its_neighbours():
    rows = _rows(3, 33, seed=4)
    for r in rows:
        r[:] = np.clip(r, np.float32(0.2), None)
    rows[0][5], rows[2][7] = np.float32(0.0625), np.float32(0.0625)
    rows[1][20] = np.float32(0.0)                       # the middle row's own best is elsewhere, and counts for nothing
    got = track.track_host(rows, [1.0, 0.0, 1.0], 0.25, 0.0, 1)
    assert got.cost == 0.125 and got.row_own_index.tolist() == [5, 20, 7]
    assert got.shifts[0] == 5 and got.shifts[2] == 7 and got.shifts[1] in (5, 6, 7)
    assert got.shifts.tolist() == [5, 6, 7]             # 7 <- 6 (the smaller |d| first: 0 is not 0.0625; -1 is) <- 5
    assert got.moves[2, 7] == -1 and got.moves[1, 6] == -1


@pytest.mark.parametrize("method", METHODS)
def test_a_reach_beyond_the_axis(method):
    rows = _rows(4, 7, seed=12, method=method)
    wide = track.track_host(rows, [1.0] * 4, 0.25, 2.0 ** -6, [0, 7, 1024, 64], method)
    same = track.track_host(rows, [1.0] * 4, 0.25, 2.0 ** -6, 6, method)
    assert wide.shifts.tolist() == same.shifts.tolist() and (_bits64(wide.row_min) == _bits64(same.row_min)).all()
    assert wide.moves.tolist() == same.moves.tolist()
    shifts, cost, row_min, row_arg, moves = _loop(rows, [1.0] * 4, 0.25, 2.0 ** -6, [0, 7, 1024, 64], method)
    assert wide.shifts.tolist() == shifts and wide.moves.tolist() == moves and _bits64(wide.cost) == _bits64(cost)
    one = track.track_host([r[:1] for r in rows], [1.0] * 4, 0.25, 0.5, 1024, method)
    assert one.shifts.tolist() == [0] * 4 and one.moves.tolist() == [[0]] * 4


@pytest.mark.parametrize("method", METHODS)
def test_penalty_extremes(method):
    E, n = 9, 257
    rows = _rows(E, n, seed=77, method=method)            # (tie-free: 257 random float32 values a row)
    weights = [1.0, 0.5, 2.0] * 3
    own = [_first(r, method) for r in rows]
    free = track.track_host(rows, weights, 0.0, 0.5, 3, method)          # lam = 0: a jump is free, every event its lone answer
    assert free.shifts.tolist() == own == free.row_own_index.tolist()
    # a huge penalty and free moves: the shift never jumps, and walks at most reach a row -- the minimum over all such walks
    rigid = track.track_host(rows, weights, 1e30, 0.0, 2, method)
    words = [int(rigid.moves[e, rigid.shifts[e]]) for e in range(1, E)]
    assert JUMP not in words and all(abs(w) <= 2 for w in words)
    assert [int(b - a) for a, b in zip(rigid.shifts[:-1], rigid.shifts[1:])] == [-w for w in words]
    D = None
    for e in range(E):
        u = [weights[e] * (-float(rows[e][j]) if method == "ccoeff_normed" else float(rows[e][j])) for j in range(n)]
        D = u if e == 0 else [u[j] + min(D[max(0, j - 2):j + 3]) for j in range(n)]
    assert _bits64(rigid.cost) == _bits64(min(D))
    # ... and with reach 0 as well: one shift, the segmentation pass's
    assert track.track_host(rows, weights, 1e30, 0.0, 0, method).shifts.tolist() == \
        segments.path_host(rows, weights, 1e30, method).shifts.tolist()


def test_track_host_refuses_bad_arguments():
    r = np.zeros(4, np.float32)
    for rows, weights in (([], []), ([r], [1.0, 1.0]), ([r, np.zeros(5, np.float32)], [1, 1]), ([r.astype(np.float64)], [1.0]),
                          ([np.zeros(0, np.float32)], [1.0]), ([r], [-1.0]), ([r], [float("nan")]), ([r.reshape(1, 4)], [1.0])):
        with pytest.raises(SushiError):
            track.track_host(rows, weights, 0.5, 0.0, 1)
    for lam in (-0.5, float("nan"), float("inf"), "much", None):
        with pytest.raises(SushiError):
            track.track_host([r], [1.0], lam, 0.0, 1)
        with pytest.raises(SushiError):
            track.track_host([r], [1.0], 0.5, lam, 1)
    with pytest.raises(SushiError):
        track.track_host([r], [1.0], 0.5, 0.0, 1, "sqdiff")
    for reach in ([0, 1025], [0, -1], [0, 1, 1], "wide", [0, None]):
        with pytest.raises(SushiError):
            track.track_host([r, r], [1.0, 1.0], 0.5, 0.0, reach)
    with pytest.raises(SushiError) as e:
        track.track_host([r, r, r], [1.0] * 3, 0.5, 0.0, [0, 5, 1025])
    assert "event 2" in str(e.value) and "1025" in str(e.value)
    assert track.track_host([r, r], [1.0, 1.0], 0.5, 0.0, [5000, 1024]).shifts.tolist() == [0, 0]      # row 0's is ignored


def test_reach_from_a_rate_and_runs_without_a_jump():
    assert track.rate_reach([100, 14500, 14500, 900], 6e-3, 1) == [0, 88, 1, 83]
    assert track.rate_reach([7], 1.0) == [0] and track.rate_reach([0, 1000], 0.0, 0) == [0, 0]
    for bad in (dict(max_rate=-1e-3), dict(max_rate=float("nan")), dict(max_rate="fast"), dict(slack=-1)):
        kw = dict(max_rate=1e-3, slack=1)
        kw.update(bad)
        with pytest.raises(SushiError):
            track.rate_reach([0, 10], kw["max_rate"], kw["slack"])
    assert track.jump_runs(5, []) == [(0, 5)] and track.jump_runs(5, [2, 3]) == [(0, 2), (2, 1), (3, 2)]
    assert track.jump_runs(1, []) == [(0, 1)]


# ---------------------------------------------------------------------------------------------- the kernels' header on the CPU
EXPECTED_RC = {   # case of host_track_check validate -> what stage_track returns
    "good": 0, "good_ccoeff": 0, "null_rows": -1, "null_reach": -1, "null_mem": -1, "method_2": -1, "method_neg": -1, "no_rows": -1,
    "negative_rows": -1, "no_shift": -1, "negative_shift": -1, "empty_curves": -1, "negative_curves": -1, "shift_beyond_curves": -1,
    "whole_sequence": 0, "rows_end_at_sequence_end": 0, "rows_past_sequence_end": -1, "row0_negative": -1, "row0_at_end": -1,
    "no_total": -1, "negative_total": -1, "rows_end_at_int_max": 0, "rows_sum_overflows_int": -1, "row0_int_max": -1,
    "row_before_curves": -1, "row_ends_at_curves_end": 0, "row_one_past_curves_end": -1, "single_shift_last_float": 0,
    "single_shift_past_end": -1, "row_at_int64_max": -1, "row_sum_overflows": -1, "huge_curves_row_at_end": 0,
    "huge_curves_row_past_end": -1, "huge_curves_int32_max_shifts": 0, "weight_nan": -1, "weight_inf": -1, "weight_negative": -1,
    "weight_neg_zero": 0, "penalty_nan": -1, "penalty_inf": -1, "penalty_negative": -1, "penalty_zero": 0, "penalty_large": 0,
    "step_cost_nan": -1, "step_cost_inf": -1, "step_cost_neg_inf": -1, "step_cost_negative": -1, "step_cost_zero": 0,
    "step_cost_neg_zero": 0, "step_cost_large": 0, "reach_all_widest": 0, "reach_1025": -1, "reach_negative": -1,
    "reach_of_a_later_calls_first_row": -1, "reach_int_max": -1, "reach_int_min": -1, "reach_of_row_0_is_ignored": 0,
    "negative_reach_of_row_0_is_ignored": 0, "reach_of_row_1": -1, "workspace_exact": 0, "workspace_short": -4, "workspace_none": -4,
    "workspace_misaligned": -2, "workspace_misaligned_and_short": -2, "bad_reach_before_workspace": -1,
    "bad_step_cost_before_alignment": -1}


def test_stage_track_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = dict(l.split() for l in lines[:len(EXPECTED_RC)])
    assert {k: int(v) for k, v in got.items()} == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    # two sets of one record of 20 bytes per workgroup, each set padded to 256 bytes; nothing for counts that make no call
    assert rest[0] == "bytes 512 512 %d %d 0 0 0" % (2 * 9472, 2 * 40960)
    # halo rounds of 256 values: none at reach 0, two up to reach 256, eight up to 1024 (2048 values)
    assert rest[1] == "halo 0 2 2 8 8 2048"
    # a tile is the item's values and the reach on each side, 8 bytes each: at most (2048 + 2048) x 8 = 32 KiB
    assert rest[2] == "tile 0 %d %d %d %d" % (514 * 8, 2560 * 8, 2080 * 8, 32768)
    assert rest[3] == "facts_one rc=0 per=2 items=1 grid=1 set=256 bytes=512 offsets=(0,8,12,16)"
    assert rest[4] == "facts_512 rc=0 per=2 items=1 grid=1 set=256 bytes=512 offsets=(0,8,12,16)"
    assert rest[5] == "facts_513 rc=0 per=2 items=2 grid=2 set=256 bytes=512 offsets=(0,16,24,32)"
    assert rest[6] == "facts_240001 rc=0 per=2 items=469 grid=469 set=9472 bytes=18944 offsets=(0,3752,5628,7504)"
    assert rest[7].startswith("facts_large_items rc=0 per=8 items=1024 grid=1024 ")
    assert rest[8].startswith("facts_small_items rc=0 per=2 items=4092 grid=2048 ")
    assert rest[9].startswith("facts_2880001 rc=0 per=8 items=1407 grid=1407 ")
    assert rest[10].startswith("facts_int32_max rc=0 per=8 items=1048576 grid=2048 set=40960 bytes=81920 ")
    assert len(rest) == 11 and cases.PER_LARGE_FROM == 1023 * 2048 + 1


def _run_check(check, tmp_path, method, lam, mu, n, curves, rows, reach):
    rt = np.array(rows, dtype=_native.JOINT_ROW_DTYPE)
    paths = [os.path.join(str(tmp_path), name) for name in ("curves", "rows", "reach", "out")]
    curves.tofile(paths[0])
    rt.tofile(paths[1])
    np.array(reach, np.int32).tofile(paths[2])
    subprocess.check_call([check, "pass", method.split("_")[0], float(lam).hex(), float(mu).hex(), str(n)] + paths)
    raw = np.fromfile(paths[3], np.uint8)
    E = len(rows)
    shifts, row_arg, own_idx = (raw[4 * E * k:4 * E * (k + 1)].view(np.int32) for k in range(3))
    own_val = raw[12 * E:16 * E].view(np.uint32)
    row_min = raw[16 * E:24 * E].view(np.uint64)
    return shifts, row_arg, own_idx, own_val, row_min, raw[24 * E:].view(np.int16).reshape(E, n)


def _compare_with_track_host(got, rows, weights, lam, mu, reach, method):
    shifts, row_arg, own_idx, own_val, row_min, moves = got
    want = track.track_host(rows, weights, lam, mu, reach, method)
    assert shifts.tolist() == want.shifts.tolist() and row_arg.tolist() == want.row_arg.tolist()
    assert own_idx.tolist() == want.row_own_index.tolist() and (own_val == _bits(want.row_own_scores)).all()
    assert (row_min == _bits64(want.row_min)).all()
    assert (moves == want.moves).all()
    return want


@pytest.mark.parametrize("method", METHODS)
def test_the_header_on_the_cpu_equals_track_host(check, tmp_path, method):
    """path_cost, track_price, track_cand, track_replaces, track_step, both first-extremum rules and track_backtrack, run by a
    program of its own over the sequences of the GPU test but the longest (ties across a workgroup boundary and in the last element,
    an all-ones sequence, weights 1, 1/3, 0 and 2.5, odd offsets, a reach that varies by row, wider than an item and wider than the
    axis) -- divided as the kernels divide them, every open order taken backwards."""
    moved = False
    for E, n, reach in cases.SHAPES[:-1] + [(4, 1025, 600), (3, 5, 1024)]:
        curves, rows, weights, lam, rs, mu = cases.sequence(E, n, reach, method, seed=3)
        want = _compare_with_track_host(_run_check(check, tmp_path, method, lam, mu, n, curves, rows, rs), cases.rows_of(curves, rows, n),
                                        weights, lam, mu, rs, method)
        words = [int(want.moves[e, want.shifts[e]]) for e in range(1, E)]
        moved |= any(w not in (0, JUMP) for w in words)
        if (E, n) == (9, 65):
            assert want.shifts.tolist() == [0] * 9 and not want.moves.any()
    assert moved


def test_the_header_on_the_cpu_on_cases_written_here(check, tmp_path):
    for method in METHODS:
        for centre in (511, 512):
            a, b = cases.tie_rows(1024, centre, method)
            curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b])
            rows = [(1, 1.0), (1027, 1.0)]
            want = _compare_with_track_host(_run_check(check, tmp_path, method, 0.5, 0.0, 1024, curves, rows, [0, 3]), [a, b],
                                            [1.0, 1.0], 0.5, 0.0, [0, 3], method)
            assert want.moves[1, centre] == -1 and want.moves[1, 0] == 0 and want.moves[1, 1023] == 0
    # the move / jump tie and one ulp above it; -0.0 through d = 0 under ccoeff; a sum a fused multiply-add would change:
    # mu * 3 with mu = 1/3 rounds to 1, and -1 + 1 is 0 where a fused form leaves -2^-54 (which would not tie with the 0.0 beside it)
    up = np.nextafter(np.float32(0.5), np.float32(1.0))
    curves = np.array([0.25, 0.5, 1.0, 0.75, 0.75, 0.0, 0.25, up, 1.0, -0.5, 0.0, -0.0, 0.0, -0.5, 0.0, 0.0, 0.0], np.float32)
    for method in METHODS:
        for rows, n, lam, mu, reach in (([(0, 1.0), (3, 1.0)], 3, 0.5, 0.25, [0, 1]), ([(6, 1.0), (3, 1.0)], 3, 0.5, 0.25, [0, 1]),
                                        ([(9, 1.0), (13, 1.0)], 4, 0.5, 0.0, [0, 1]), ([(0, 1.0), (1, 0.0), (2, 1.0)], 2, 0.25, 0.125, [0, 1, 1])):
            got = _run_check(check, tmp_path, method, lam, mu, n, curves, rows, reach)
            _compare_with_track_host(got, cases.rows_of(curves, rows, n), [w for _o, w in rows], lam, mu, reach, method)
    fma = _run_check(check, tmp_path, "sqdiff_normed", 4.0, 1.0 / 3.0, 4, np.array([0, 5, 5, -1, 0, 0, 0, 0], np.float32),
                     [(0, 1.0), (4, 1.0)], [0, 3])
    # D_0 = [0, 5, 5, -1]: at j = 0, cand(0) = 0.0 and cand(+3) = -1 + 1 = 0.0: the tie keeps d = 0 (a fused form would move by 3)
    assert fma[5][1].tolist() == [0, 2, 1, 0] and fma[4].tolist() == _bits64([-1.0, -1.0]).tolist()


# ---------------------------------------------------------------------------------------------- the entry points, no GPU
def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    assert {"sushi_hip_track_bytes", "sushi_hip_track_forward", "sushi_hip_track_backtrack"} <= set(_native.declared_symbols())
    assert (_native.TRACK_MAX_REACH, _native.TRACK_JUMP) == (1024, -32768)
    assert L.sushi_hip_track_bytes(1, 1) == 512 and L.sushi_hip_track_bytes(200, 240001) == 18944
    assert L.sushi_hip_track_bytes(0, 5) == 0 and L.sushi_hip_track_bytes(5, 0) == 0 and L.sushi_hip_track_bytes(-1, -1) == 0
    rows = np.array([(0, 1.0), (501, 0.0), (333, 2.5)], dtype=_native.JOINT_ROW_DTYPE)
    reach = np.array([0, 1024, 17], np.int32)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)

    def call(curves=P, n_curve=1000, rows=rows, reach=reach, n_rows=3, n_shift=499, method=0, penalty=0.5, step_cost=1e-3, row0=2,
             n_total=7, outs=(P, P, P, P, P, P), mem=P, mem_bytes=1 << 16):
        return L.sushi_hip_track_forward(curves, n_curve, None if rows is None else rows.ctypes.data,
                                         None if reach is None else reach.ctypes.data, n_rows, n_shift, method, penalty, step_cost,
                                         row0, n_total, *outs, mem, mem_bytes, None)

    EINVAL, EALIGN = -1, -2
    assert call(curves=None) == EINVAL and call(rows=None) == EINVAL and call(reach=None) == EINVAL and call(mem=None) == EINVAL
    for k in range(6):
        assert call(outs=tuple(None if i == k else P for i in range(6))) == EINVAL
    assert call(method=2) == EINVAL and call(method=-1) == EINVAL
    assert call(n_rows=0) == EINVAL and call(n_shift=0) == EINVAL and call(n_curve=0) == EINVAL and call(n_shift=1001) == EINVAL
    assert call(row0=-1) == EINVAL and call(row0=5) == EINVAL and call(n_total=0) == EINVAL and call(row0=7) == EINVAL
    assert call(row0=2 ** 31 - 3, n_total=2 ** 31 - 1) == EINVAL          # row0 + n_rows would pass int: never formed
    for bad in (np.nan, np.inf, -1e-300):
        assert call(penalty=bad) == EINVAL and call(step_cost=bad) == EINVAL
    for at, value in ((0, 1025), (1, 1025), (2, -1), (1, 2 ** 31 - 1)):
        r = reach.copy()
        r[at] = value
        assert call(reach=r) == EINVAL, (at, value)
    r = reach.copy()
    r[0] = 5000
    assert call(reach=r, row0=0, mem_bytes=16) == _native.ENOSPACE        # the sequence's row 0: its reach is ignored
    for field, at, value in (("curve_off", 0, -1), ("curve_off", 1, 502), ("curve_off", 2, 2 ** 63 - 1), ("weight", 0, np.nan),
                             ("weight", 1, np.inf), ("weight", 2, -1.0)):
        bad = rows.copy()
        bad[field][at] = value
        assert call(rows=bad) == EINVAL, (field, at, value)
    huge = rows.copy()
    huge["curve_off"][2] = 2 ** 63 - 500
    assert call(rows=huge, n_curve=2 ** 63 - 1, mem_bytes=16) == _native.ENOSPACE    # valid at int64's end; the workspace is what fails
    assert call(mem=odd(128)) == EALIGN and call(mem_bytes=511) == _native.ENOSPACE and call(mem_bytes=0) == _native.ENOSPACE
    assert call(curves=odd(2)) == EALIGN
    for k, off in enumerate((4, 1, 4, 2, 2, 2)):      # D, row_min: 8 bytes; moves: 2; row_arg, row_own_index, row_own_score: 4
        assert call(outs=tuple(odd(off) if i == k else P for i in range(6))) == EALIGN, k

    def back(moves=P, row_arg=P, n_total=7, n_shift=499, out=P):
        return L.sushi_hip_track_backtrack(moves, row_arg, n_total, n_shift, out, None)

    assert back(moves=None) == EINVAL and back(row_arg=None) == EINVAL and back(out=None) == EINVAL
    assert back(n_total=0) == EINVAL and back(n_shift=0) == EINVAL and back(n_total=-1) == EINVAL
    assert back(moves=odd(1)) == EALIGN and back(row_arg=odd(2)) == EALIGN and back(out=odd(2)) == EALIGN


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


def test_find_track_refuses_on_the_host():
    stream = _NoDevice()
    patterns = [np.zeros((1, 6000), np.uint8)] * 4
    centres = [1.0, 2.0, 3.0, 20.0]
    need = 4 * 24001 * 2 + 2 * 24001 * 8
    assert track.TrackState.nbytes(4, 24001) == need and track.TrackState.nbytes(200, 240001) == 96000400 + 3840016
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, reach=4, max_state_bytes=need - 1)
    assert str(need) in str(e.value) and "max_state_bytes" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, max_rate=1e-3, max_bytes=4 * 24001 - 1)
    assert str(4 * 24001) in str(e.value)
    # 17 s between events 2 and 3 at 6e-3: ceil(0.006 * 204000) + 1 = 1225 samples: nothing is clipped silently
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, max_rate=6e-3)
    assert "event 3" in str(e.value) and "1225" in str(e.value) and "1024" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, reach=[0, 3, 1025, 3])
    assert "event 2" in str(e.value) and "1025" in str(e.value)
    for bad in (dict(), dict(max_rate=1e-3, reach=3), dict(reach=[1, 2]), dict(reach=-1), dict(max_rate=-1.0), dict(max_rate=1e-3, slack=-1),
                dict(reach=1, step_cost=-1.0), dict(reach=1, step_cost=float("nan")), dict(reach=1, weights="median"),
                dict(reach=1, weights=[1.0]), dict(reach=1, method="sqdiff")):
        with pytest.raises(SushiError):
            track.find_track(stream, patterns, centres, 1.0, 0.5, **bad)
    for lam in (-1.0, float("nan")):
        with pytest.raises(SushiError):
            track.find_track(stream, patterns, centres, 1.0, lam, reach=1)
    with pytest.raises(SushiError):
        track.find_track(stream, patterns, centres[:3], 1.0, 0.5, reach=1)
    with pytest.raises(TypeError):
        track.find_track(stream, patterns, centres, 1.0, reach=1)                 # the penalty has no default


def test_track_device_refuses_on_the_host():
    class _State(object):
        n_total, n_shift = 3, 8

        class D(object):
            device = "nowhere"

    with pytest.raises(SushiError):
        track.track_device(np.zeros(64, np.float32), [(0, 1.0)], 1, 0.5, 0.0, _State())         # curves are not a CUDA tensor
    with pytest.raises(SushiError):
        track.TrackState(0, 8, None)
    with pytest.raises(SushiError):
        track.TrackState(3, 2 ** 31, None)
    assert track.checked_reach(5, 3).tolist() == [0, 5, 5] and track.checked_reach([9, 1024], 2, first_row=4).tolist() == [9, 1024]
    with pytest.raises(SushiError) as e:
        track.checked_reach([9, 1025], 2, first_row=4)
    assert "event 5" in str(e.value)


# ---------------------------------------------------------------------------------------------- the scenario on the oracle
@pytest.fixture(scope="module")
def oracle_case(oracle):
    dst, src = cases.streams()
    patterns, _centres, bases = cases.scenario(dst, src)
    k_lo, n_shift = joint.joint_window(bases, [p.shape[1] for p in patterns], dst.data.shape[1], int(cases.RATE * cases.WINDOW))
    return k_lo, n_shift, bases, cases.oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift)


def test_the_pass_follows_a_shift_the_segmentation_pass_cannot(oracle, oracle_case):
    """The oracle alone shows it: lone searches place both victims at their decoys; path_host returns those at penalty 0.1, drags
    neighbours onto the decoys at 0.25 and collapses to one shift from 0.5 on -- wrong at all five penalties; track_host returns the
    ten true shifts at every penalty from 0.1 to 1.0, with free and with priced moves, and no longer pays for the cut at 2.0."""
    k_lo, n_shift, bases, rows = oracle_case
    assert (k_lo, n_shift) == (cases.K_LO, cases.N_SHIFT)
    assert track.rate_reach(bases, cases.MAX_RATE, cases.SLACK) == cases.REACH
    lone = [oracle.argmin_first(r) + k_lo for r in rows]
    assert lone == cases.LONE_K
    for v, d in zip(cases.VICTIMS, cases.DECOYS):
        assert lone[v] == cases.TRUE_K[v] + d
    assert [lam for lam, _s, _c in cases.PATH_RESULTS] == list(cases.PATH_PENALTIES)
    for lam, shifts, cost in cases.PATH_RESULTS:
        got = segments.path_host(rows, [1.0] * 10, lam)
        assert (got.shifts + k_lo).tolist() == shifts and got.cost == cost, lam
        assert (got.shifts + k_lo).tolist() != cases.TRUE_K
    assert sorted(cases.TRACK_COSTS) == sorted(itertools.product(cases.TRACK_PENALTIES, cases.STEP_COSTS))
    for (lam, mu), cost in cases.TRACK_COSTS.items():
        got = track.track_host(rows, [1.0] * 10, lam, mu, cases.REACH)
        assert (got.shifts + k_lo).tolist() == cases.TRUE_K and got.cost == cost, (lam, mu)
        assert [e for e in range(1, 10) if got.moves[e, got.shifts[e]] == JUMP] == cases.JUMPS
    got = track.track_host(rows, [1.0] * 10, cases.PENALTY, 0.0, cases.REACH)
    assert _bits([r[s] for r, s in zip(rows, got.shifts)]).tolist() == cases.EVENT_SCORE_BITS
    assert (got.row_own_index + k_lo).tolist() == cases.LONE_K and _bits(got.row_own_scores).tolist() == cases.OWN_SCORE_BITS
    far = track.track_host(rows, [1.0] * 10, cases.PENALTY_TOO_LARGE, 0.0, cases.REACH)
    assert (far.shifts + k_lo).tolist() == cases.TOO_LARGE_K != cases.TRUE_K
