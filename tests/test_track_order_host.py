"""Ordered tracking without a GPU: the NumPy restatement of sushi_hip_track_forward_ordered / sushi_hip_track_backtrack_ordered
(sushi_amd/track.py track_ordered_host) against the recursion written out on Python floats and against a brute force over all
assignments, against today's pass where the backs set no limit, planted ties of the prefix minimum, the kernels' own header
compiled for the CPU (tests/host_track_order_check.cpp, a program of its own under AddressSanitizer + UBSan), the argument checks,
and the decoy scenario on the CPU oracle: what the feature is for."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import track_cases
import track_order_cases as cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, joint, track
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, chapter_penalties

METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP, ANY = -32768, -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("track_order_check")), "host_track_order_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_track_order_check.cpp"), "-o", exe])
    return exe


def _t(j, back, n):
    return n - 1 if back < 0 else min(j + back, n - 1)


def _loop(rows, weights, lams, mu, reach, back, method):
    """The definition, written out: one shift and one candidate at a time on Python floats (IEEE float64), the prefix minimum by a
    scan upwards with a strict <.  -> (shifts, cost, row_min, row_arg, moves, prefix_arg)"""
    E, n = len(rows), rows[0].shape[0]
    D, moves, row_min, row_arg, args = None, [[0] * n], [], [], []
    for e in range(E):
        u = [float(weights[e]) * (-float(rows[e][j]) if method == "ccoeff_normed" else float(rows[e][j])) for j in range(n)]
        if e == 0:
            D = u
        else:
            A = args[e - 1]
            new, mv = [], []
            for j in range(n):
                cands = [(D[j], 0, False)]
                for d in range(-reach[e], reach[e] + 1):
                    if d != 0 and 0 <= j + d < n:
                        cands.append((D[j + d] + mu * float(abs(d)), abs(d), d > 0))
                near, ad, pos = min(cands)
                jump = D[A[_t(j, back[e], n)]] + float(lams[e])
                take = near <= jump
                new.append(u[j] + (near if take else jump))
                mv.append((ad if pos else -ad) if take else JUMP)
            D = new
            moves.append(mv)
        A, at = [], 0
        for t in range(n):
            if D[t] < D[at]:
                at = t
            A.append(at)
        args.append(A)
        row_arg.append(A[n - 1])
        row_min.append(D[A[n - 1]])
    s = row_arg[-1]
    shifts = [s]
    for e in range(E - 1, 0, -1):
        s = args[e - 1][_t(s, back[e], n)] if moves[e][s] == JUMP else s + moves[e][s]
        shifts.append(s)
    return shifts[::-1], row_min[-1], row_min, row_arg, moves, args


def _rows(E, n, seed, method="sqdiff_normed"):
    rng = np.random.default_rng(seed)
    lo = 0.0 if method == "sqdiff_normed" else -1.0
    return [(rng.random(n, dtype=np.float32) * np.float32(1.0 - lo) + np.float32(lo)).astype(np.float32) for _ in range(E)]


def _path_cost(rows, weights, lams, mu, reach, back, method, path):
    """A path's cost accumulated in the pass's order: c = u_0[s_0]; per event the cheapest allowed choice of c + mu |d| (a move
    within reach; c itself for d = 0) and c + lam_e (a jump, allowed where s_e >= s_{e-1} - back_e), then c = u_e[s_e] + c; inf
    where an event can be entered neither way."""
    u = lambda e: float(weights[e]) * (-float(rows[e][path[e]]) if method == "ccoeff_normed" else float(rows[e][path[e]]))
    c = u(0)
    for e in range(1, len(rows)):
        d = abs(path[e] - path[e - 1])
        choices = []
        if back[e] < 0 or path[e] >= path[e - 1] - back[e]:
            choices.append(c + float(lams[e]))
        if d == 0:
            choices.append(c)
        elif d <= reach[e]:
            choices.append(c + mu * float(d))
        if not choices:
            return float("inf")
        c = u(e) + min(choices)
    return c


# ---------------------------------------------------------------------------------------------- track_ordered_host
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("E", [1, 2, 7, 33])
@pytest.mark.parametrize("n", [1, 63, 65, 513])
def test_track_ordered_host_is_the_recursion_written_out(E, n, method):
    for reach in (0, 1, 3, 64):
        rows = _rows(E, n, seed=E * 10007 + n + reach, method=method)
        rs = [reach] * E if reach < 2 else track_cases.reaches(E, reach)
        weights, lam, mu = (([1.0] * E, 0.25, 2.0 ** -7), ([(1.0 / 3.0, 0.0, 2.5)[i % 3] for i in range(E)], 1.0 / 3.0, 1e-3),
                            ([1.0] * E, 0.125, 0.0), ([1.0] * E, 0.0, 0.01))[(reach + E) % 4]
        lams, back = cases.penalties(E, lam), cases.backs(E, n)
        got = track.track_ordered_host(rows, weights, lams, mu, rs, back, method)
        shifts, cost, row_min, row_arg, moves, args = _loop(rows, weights, lams, mu, [0] + list(rs[1:]), back, method)
        assert got.shifts.tolist() == shifts and got.row_arg.tolist() == row_arg, (reach,)
        assert (_bits64(got.row_min) == _bits64(row_min)).all() and _bits64(got.cost) == _bits64(cost)
        assert got.moves.tolist() == moves and got.prefix_arg.tolist() == args
        assert got.shifts.dtype == np.int32 and got.moves.dtype == np.int16 and got.prefix_arg.dtype == np.int32
        assert got.prefix_arg.shape == (E, n)


@pytest.mark.parametrize("method", METHODS)
def test_the_pass_finds_the_minimum_over_all_ordered_paths(method):
    """E <= 4, n_shift <= 6, reach 0 / 1, backs 0, 1, n and no limit mixed, penalties mixed, dyadic values (every sum exact, so ties
    are real ties): track_ordered_host's cost is the minimum over all n_shift^E paths of the in-order cost, exactly, its own path
    attains it, and every jump of that path obeys its back."""
    rng = np.random.default_rng(16)
    sign = -1.0 if method == "ccoeff_normed" else 1.0
    seen_move = seen_jump = seen_bound = False
    for E, n in itertools.product((1, 2, 3, 4), (1, 2, 3, 6)):
        for trial in range(8):
            rows = [(sign * rng.integers(0, 17, n) / 16.0).astype(np.float32) for _ in range(E)]
            weights = [(1.0, 0.5, 2.0, 0.0)[int(k)] for k in rng.integers(0, 4, E)]
            lams = [(0.0, 0.125, 0.5, 1.0, 4.0, 0.3, 0.25, 2.0)[int(k)] for k in rng.integers(0, 8, E)]
            mu = (0.0, 0.0625, 0.25, 0.125, 1.0, 0.1, 0.0, 0.5)[(trial + E) % 8]
            reach = [int(k) for k in rng.integers(0, 2, E)]
            back = [(0, 1, n, ANY)[int(k)] for k in rng.integers(0, 4, E)]
            got = track.track_ordered_host(rows, weights, lams, mu, reach, back, method)
            reach[0] = 0
            costs = [_path_cost(rows, weights, lams, mu, reach, back, method, p) for p in itertools.product(range(n), repeat=E)]
            assert got.cost == min(costs), (E, n, trial)
            path = got.shifts.tolist()
            assert _path_cost(rows, weights, lams, mu, reach, back, method, path) == got.cost, (E, n, trial)
            words = [int(got.moves[e, path[e]]) for e in range(1, E)]
            for e in range(1, E):
                if words[e - 1] == JUMP and back[e] >= 0:
                    assert path[e] >= path[e - 1] - back[e]
            seen_bound |= track.track_ordered_host(rows, weights, lams, mu, reach, ANY, method).cost < got.cost   # a back that binds
            seen_move |= any(w not in (0, JUMP) for w in words)
            seen_jump |= JUMP in words
    assert seen_move and seen_jump and seen_bound


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", track_cases.SHAPES)
def test_without_a_limit_it_is_todays_pass(shape, method):
    """Every back without a limit, and again every back >= n_shift - 1, and one penalty: shifts, cost, row_min, row_arg and moves are
    track_host's, bitwise."""
    E, n, reach = shape
    curves, rows, weights, lam, rs, mu = track_cases.sequence(E, n, reach, method, seed=3)
    R = track_cases.rows_of(curves, rows, n)
    want = track.track_host(R, weights, lam, mu, rs, method)
    for back in (ANY, None, [ANY] * E, n - 1, [n - 1 + (e % 3) for e in range(E)], 2 ** 31 - 1):
        got = track.track_ordered_host(R, weights, lam, mu, rs, back, method)
        assert got.shifts.tolist() == want.shifts.tolist() and got.row_arg.tolist() == want.row_arg.tolist()
        assert (_bits64(got.row_min) == _bits64(want.row_min)).all() and _bits64(got.cost) == _bits64(want.cost)
        assert (got.moves == want.moves).all()
        assert got.row_own_index.tolist() == want.row_own_index.tolist()
        assert (_bits(got.row_own_scores) == _bits(want.row_own_scores)).all()
        assert got.prefix_arg[:, n - 1].tolist() == want.row_arg.tolist()


# ---------------------------------------------------------------------------------------------- planted ties
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("at", [256, 512])
def test_equal_minima_on_both_sides_of_a_tile_boundary(at, method):
    """D_0's minimum twice, at at - 1 | at: A is the lower index from at - 1 on, and a jump from beyond goes there."""
    a, b = cases.prefix_tie_rows(1024, at, method)
    got = track.track_ordered_host([a, b], [1.0, 1.0], 0.0625, 0.0, 0, [ANY, 0], method)
    A = got.prefix_arg[0]
    assert A[at - 1] == at - 1 and A[at] == at - 1 and A[1023] == at - 1 and A[0] == 0
    assert (np.diff(A) >= 0).all() and (A <= np.arange(1024)).all()
    assert got.moves[1, at + 1] == JUMP and got.moves[1, at] == 0 and got.moves[1, at - 1] == 0 and got.moves[1, 1023] == JUMP
    # back 0: a jump into j comes from A[j]; just above the tie the source is the lower of the two
    s = int(got.shifts[1])
    assert got.shifts[0] == (A[s] if got.moves[1, s] == JUMP else s)
    forced = track.backtrack_ordered_host(got.moves, got.prefix_arg, np.array([ANY, 0], np.int32), np.array([0, at + 1], np.int32))
    assert forced.tolist() == [at - 1, at + 1]


def test_a_decreasing_row_and_an_increasing_one():
    n = 300
    down = np.linspace(0.75, 0.25, n).astype(np.float32)        # strictly decreasing: every index is a record
    up = down[::-1].copy()                                      # strictly increasing: index 0 is the only one
    flat = np.full(n, 0.5, np.float32)
    got = track.track_ordered_host([down, flat], [1.0, 1.0], 0.0, 0.0, 0, [ANY, 0])
    assert got.prefix_arg[0].tolist() == list(range(n)) and got.prefix_arg[1].tolist() == list(range(n))
    assert not (got.moves[1] == JUMP).any()                     # back 0: P[j] is D[j] itself, and the tie moves
    got = track.track_ordered_host([down, flat], [1.0, 1.0], 0.0, 0.0, 0, [ANY, 5])
    assert (got.moves[1, :n - 1] == JUMP).all() and got.moves[1, n - 1] == 0       # ... from 5 further up, but for the last one
    got = track.track_ordered_host([up, flat], [1.0, 1.0], 0.0, 0.0, 0, [ANY, 0])
    assert got.prefix_arg[0].tolist() == [0] * n and got.moves[1].tolist() == [0] + [JUMP] * (n - 1)
    assert got.shifts.tolist() == [0, 0]


def test_a_tie_between_moving_and_jumping_moves_and_a_penalty_of_zero():
    # D_0 = [0.25, 0.5, 1.0], mu = 0.25, lam = 0.5: at j = 2, near = 0.5 + 0.25 = jump = 0.25 + 0.5: the tie moves, by -1
    rows = [np.array([0.25, 0.5, 1.0], np.float32), np.array([0.75, 0.75, 0.0], np.float32)]
    got = track.track_ordered_host(rows, [1.0, 1.0], [9.0, 0.5], 0.25, 1, [ANY, 0])
    assert got.moves[1].tolist() == [0, 0, -1] and got.shifts.tolist() == [1, 2] and got.row_min.tolist() == [0.25, 0.75]
    rows[0] = np.array([0.25, np.nextafter(np.float32(0.5), np.float32(1.0)), 1.0], np.float32)
    got = track.track_ordered_host(rows, [1.0, 1.0], [9.0, 0.5], 0.25, 1, [ANY, 0])
    assert got.moves[1, 2] == JUMP and got.shifts.tolist() == [0, 2] and got.cost == 0.75
    # a penalty of 0: near == P + 0 wherever the index is a record (the tie moves: no jump), a jump everywhere else
    d0 = np.array([0.5, 0.25, 0.75, 0.25, 0.125], np.float32)
    got = track.track_ordered_host([d0, np.zeros(5, np.float32)], [1.0, 1.0], 0.0, 0.0, 0, [ANY, 0])
    assert got.prefix_arg[0].tolist() == [0, 1, 1, 1, 4] and got.moves[1].tolist() == [0, 0, JUMP, 0, 0]
    assert got.row_min.tolist() == [0.125, 0.125] and got.shifts.tolist() == [4, 4]


def test_back_zero_at_the_last_index_and_a_back_beyond_the_axis():
    d0 = np.array([0.5, 0.125, 0.75, 0.25], np.float32)
    d1 = np.array([0.5, 0.5, 0.5, 0.0], np.float32)
    got = track.track_ordered_host([d0, d1], [1.0, 1.0], 0.0625, 0.0, 0, [ANY, 0])
    # t(3) = min(3 + 0, 3) = 3: P[3] = D_0[1]
    assert got.moves[1, 3] == JUMP and got.shifts.tolist() == [1, 3] and got.cost == 0.125 + 0.0625
    # into j = 0 nothing but 0 itself: the best path that ends there stays
    assert got.moves[1, 0] == 0 and got.prefix_arg[0].tolist() == [0, 1, 1, 1]
    # an event that would have to go back cannot: the minimum is at 3 in row 0, at 0 in row 1
    back0 = track.track_ordered_host([d1, d0[::-1].copy()], [1.0, 1.0], 0.0625, 0.0, 0, [ANY, 0])
    free = track.track_ordered_host([d1, d0[::-1].copy()], [1.0, 1.0], 0.0625, 0.0, 0, [ANY, 1])
    assert free.shifts.tolist() == [3, 2] and free.cost == 0.125 + 0.0625
    assert back0.shifts.tolist() == [3, 3] and back0.cost == 0.5
    for big in (4, 11, 2 ** 31 - 1):
        assert track.track_ordered_host([d0, d1], [1.0, 1.0], 0.0625, 0.0, 0, [ANY, big]).moves.tolist() == \
            track.track_ordered_host([d0, d1], [1.0, 1.0], 0.0625, 0.0, 0, ANY).moves.tolist()


def test_negative_zero_travels_through_the_prefix_minimum():
    """A row of weight 0 under 'ccoeff_normed': u = 0 * -(x) = -0.0 for x > 0 and 0.0 for x < 0.  P is D[A] itself: with D_0 = [0.0,
    -0.0, -0.0] the prefix minimum is 0.0 (index 0: the zeros tie) at every t, not -0.0; with D_0 = [-0.0, 0.0, 0.0] it is -0.0."""
    pos, neg = np.array([-0.5, 0.5, 0.5], np.float32), np.array([0.5, -0.5, -0.5], np.float32)
    nxt = np.array([-0.25, -0.25, -0.25], np.float32)
    for first, sign_bit in ((pos, 0), (neg, 1)):
        got = track.track_ordered_host([first, nxt], [0.0, 0.0], 0.0, 0.0, 0, [ANY, ANY], "ccoeff_normed")
        assert got.prefix_arg[0].tolist() == [0, 0, 0] and _bits64(got.row_min[0]) == sign_bit << 63
        # row 1: index 0 stays (a tie moves); 1 and 2 tie with the jump as well (0.0 == -0.0) and stay
        assert got.moves[1].tolist() == [0, 0, 0]
    # with a penalty the jump loses; with a negative u first the prefix minimum is what a jump adds the penalty to
    got = track.track_ordered_host([neg, nxt], [0.0, 1.0], 0.0, 0.0, 0, [ANY, ANY], "ccoeff_normed")
    assert _bits64(got.row_min[0]) == 1 << 63 and got.row_min[1] == 0.25 and got.shifts.tolist() == [0, 0]
    # D_0 = [0.0, -0.0, -0.0] with a jump forced by an ulp: P + 0 = 0.0 + 0.0 = 0.0 where D_0[j] = -0.0 itself would have stayed
    a = np.array([-0.5, 0.5, 0.5], np.float32)
    want = _loop([a, nxt], [0.0, 0.0], [0.0, 0.0], 0.0, [0, 0], [ANY, ANY], "ccoeff_normed")
    got = track.track_ordered_host([a, nxt], [0.0, 0.0], 0.0, 0.0, 0, ANY, "ccoeff_normed")
    assert (_bits64(got.row_min) == _bits64(want[2])).all() and got.moves.tolist() == want[4]


# ---------------------------------------------------------------------------------------------- the scenario on the oracle
@pytest.fixture(scope="module")
def oracle_case(oracle):
    dst, src = cases.streams()
    patterns, _centres, bases = cases.scenario(dst, src)
    lens = [p.shape[1] for p in patterns]
    k_lo, n_shift = joint.joint_window(bases, lens, dst.data.shape[1], int(cases.RATE * cases.WINDOW))
    return k_lo, n_shift, bases, lens, cases.oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift)


def test_the_ordered_pass_is_right_where_todays_follows_the_decoys(oracle, oracle_case):
    """The oracle alone shows it.  At penalties 0.01 - 0.03 track_host takes the decoys -- two jumps each, one of them 8400 samples
    back across a gap of 3600 -- and the ordered pass returns the ten true shifts; at 0.05 - 0.25 both do; at 0.5 the cut no longer
    pays for either.  With every back without a limit the ordered pass is track_host at all of them."""
    k_lo, n_shift, bases, lens, rows = oracle_case
    assert (k_lo, n_shift) == (cases.K_LO, cases.N_SHIFT)
    back = track.order_back(bases, lens)
    assert [None if b == ANY else b for b in back] == cases.BACK
    assert [oracle.argmin_first(r) + k_lo for r in rows] == cases.LONE_K
    for v, d in zip(cases.VICTIMS, cases.DECOYS):
        assert cases.LONE_K[v] == cases.TRUE_K[v] + d
    assert _bits([r[k - k_lo] for r, k in zip(rows, cases.TRUE_K)]).tolist() == cases.EVENT_SCORE_BITS
    assert sorted(cases.RESULTS) == sorted(cases.PENALTIES_ORDER_ONLY + cases.PENALTIES_BOTH + (cases.PENALTY_TOO_LARGE,))
    for lam, (plain_k, plain_cost, ordered_k, ordered_cost) in sorted(cases.RESULTS.items()):
        plain = track.track_host(rows, [1.0] * 10, lam, 0.0, 0)
        ordered = track.track_ordered_host(rows, [1.0] * 10, lam, 0.0, 0, back)
        assert (plain.shifts + k_lo).tolist() == plain_k and plain.cost == plain_cost, lam
        assert (ordered.shifts + k_lo).tolist() == ordered_k and ordered.cost == ordered_cost, lam
        assert (plain_k == cases.TRUE_K) == (lam in cases.PENALTIES_BOTH)
        assert (ordered_k == cases.TRUE_K) == (lam in cases.PENALTIES_ORDER_ONLY + cases.PENALTIES_BOTH)
        if ordered_k == cases.TRUE_K:
            assert [e for e in range(1, 10) if ordered.moves[e, ordered.shifts[e]] == JUMP] == [5]
        free = track.track_ordered_host(rows, [1.0] * 10, lam, 0.0, 0, ANY)
        assert free.shifts.tolist() == plain.shifts.tolist() and _bits64(free.cost) == _bits64(plain.cost)
        assert (free.moves == plain.moves).all()
    # a penalty per event: dear everywhere but at the one gap that can hold the cut
    lams = [0.0] + [0.01 if e == 5 else 1.0 for e in range(1, 10)]
    got = track.track_ordered_host(rows, [1.0] * 10, lams, 0.0, 0, ANY)
    assert (got.shifts + k_lo).tolist() == cases.TRUE_K


# ---------------------------------------------------------------------------------------------- arguments
def test_order_back():
    assert track.order_back([100, 300, 300, 1000], [50, 250, 10, 5]) == [ANY, 150, 0, 690]
    assert track.order_back([100, 300, 300, 1000], [50, 250, 10, 5], slack=2) == [ANY, 152, 2, 692]
    assert track.order_back([7], [3]) == [ANY]
    with pytest.raises(SushiError) as e:
        track.order_back([100, 300, 299], [5, 5, 5])
    assert "event 2" in str(e.value)
    for bad in (([], []), ([1, 2], [1]), ([1, 2], [1, -1]), (["a"], [1])):
        with pytest.raises(SushiError):
            track.order_back(*bad)
    with pytest.raises(SushiError):
        track.order_back([1, 2], [1, 1], slack=-1)


def test_track_ordered_host_refuses_bad_arguments():
    r = np.zeros(4, np.float32)
    ok = track.track_ordered_host([r, r], [1.0, 1.0], [float("nan"), 0.5], 0.0, 0, [7, None])     # row 0's are not used
    assert ok.shifts.tolist() == [0, 0]
    for lams in ([0.0, -0.5], [0.0, float("nan")], [0.0, float("inf")], [0.5], [0.5, 0.5, 0.5], "much", [0.0, None], -1.0):
        with pytest.raises(SushiError):
            track.track_ordered_host([r, r], [1.0, 1.0], lams, 0.0, 0, ANY)
    with pytest.raises(SushiError) as e:
        track.track_ordered_host([r, r, r], [1.0] * 3, [0.0, 0.5, -2.0], 0.0, 0, ANY)
    assert "event 2" in str(e.value)
    for back in ([ANY, -2], [-2, 0], -2, [0], [0, 0, 0], "far", [0, "far"], [0, 2 ** 31]):
        with pytest.raises(SushiError):
            track.track_ordered_host([r, r], [1.0, 1.0], 0.5, 0.0, 0, back)
    with pytest.raises(SushiError) as e:
        track.track_ordered_host([r, r, r], [1.0] * 3, 0.5, 0.0, 0, [0, 5, -3])
    assert "event 2" in str(e.value) and "-3" in str(e.value)
    for rows, weights in (([], []), ([r], [1.0, 1.0]), ([r, np.zeros(5, np.float32)], [1, 1]), ([r], [-1.0])):
        with pytest.raises(SushiError):
            track.track_ordered_host(rows, weights, 0.5, 0.0, 1, ANY)
    with pytest.raises(SushiError):
        track.track_ordered_host([r, r], [1.0, 1.0], 0.5, -1.0, 1, ANY)
    with pytest.raises(SushiError):
        track.track_ordered_host([r, r], [1.0, 1.0], 0.5, 0.0, [0, 1025], ANY)
    assert track.checked_back(None, 3).tolist() == [ANY] * 3 and track.checked_back([None, 0, 7], 3).tolist() == [ANY, 0, 7]
    assert track.checked_penalties(0.5, 3).tolist() == [0.0, 0.5, 0.5]
    assert track.checked_penalties([0.25, 0.5], 2, first_row=4).tolist() == [0.25, 0.5]
    with pytest.raises(SushiError) as e:
        track.checked_penalties([0.25, -0.5], 2, first_row=4)
    assert "event 5" in str(e.value)


def test_chapter_penalties():
    events = [ScriptEvent(s, e) for s, e in ((1.0, 2.0), (2.5, 9.9), (9.5, 10.0), (9.8, 10.5), (11.0, 12.0), (30.0, 31.0), (31.0, 32.0))]
    # chapters from 0, 10, 20 and 30 s: an event belongs to the chapter its end falls in (an end AT a mark is still the one before)
    got = chapter_penalties(events, [0.0, 10.0, 20.0, 30.0], 1.0, 0.05)
    assert got == [1.0, 1.0, 1.0, 0.05, 1.0, 0.05, 1.0]
    assert chapter_penalties(events, [0.0], 1.0, 0.05) == [1.0] * 7 and chapter_penalties([], [0.0, 1.0], 1.0, 0.05) == []
    assert chapter_penalties(events[:1], [0.0, 1.5], 0.5, 0.25) == [0.5]
    for bad in ((-1.0, 0.5), (1.0, float("nan")), ("much", 0.5), (1.0, float("inf"))):
        with pytest.raises(SushiError):
            chapter_penalties(events, [0.0, 10.0], *bad)


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
    centres = [1.0, 2.0, 3.0, 4.0]
    for kw in (dict(order=True), dict(order=[None, 0, 0, 0]), dict(penalty=[0.0, 0.5, 0.5, 0.5])):
        args = dict(penalty=0.5, reach=0, margins=True)
        args.update(kw)
        with pytest.raises(SushiError) as e:
            track.find_track(stream, patterns, centres, 1.0, **args)
        assert "not built" in str(e.value)
    need = 4 * 24001 * 6 + 3 * 24001 * 8
    assert track.TrackState.nbytes(4, 24001, ordered=True) == need
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, reach=0, order=True, max_state_bytes=need - 1)
    assert str(need) in str(e.value) and "max_state_bytes" in str(e.value)
    for bad in (dict(order=[0, 0, 0]), dict(order=[None, 0, -2, 0]), dict(order="yes"), dict(penalty=[0.5, 0.5, 0.5]),
                dict(penalty=[0.0, 0.5, -0.5, 0.5]), dict(penalty=[0.0, 0.5, float("nan"), 0.5])):
        args = dict(penalty=0.5, reach=0)
        args.update(bad)
        with pytest.raises(SushiError):
            track.find_track(stream, patterns, centres, 1.0, **args)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, [1.0, 3.0, 2.0, 4.0], 1.0, 0.5, reach=0, order=True)       # the events are not in order
    assert "event 2" in str(e.value)
    with pytest.raises(SushiError):
        track.TrackState(3, 8, None, keep=True, ordered=True)


# ---------------------------------------------------------------------------------------------- the kernels' header on the CPU
EXPECTED_RC = {   # case of host_track_order_check validate -> what stage_track_ordered returns
    "good": 0, "good_ccoeff": 0, "null_rows": -1, "null_reach": -1, "null_mem": -1, "method_2": -1, "no_rows": -1, "no_shift": -1,
    "empty_curves": -1, "shift_beyond_curves": -1, "rows_end_at_sequence_end": 0, "rows_past_sequence_end": -1, "row0_negative": -1,
    "no_total": -1, "rows_sum_overflows_int": -1, "row_ends_at_curves_end": 0, "row_one_past_curves_end": -1, "row_at_int64_max": -1,
    "weight_nan": -1, "weight_negative": -1, "step_cost_nan": -1, "step_cost_negative": -1, "reach_1025": -1, "reach_negative": -1,
    "reach_of_row_0_is_ignored": 0, "null_back": -1, "back_all_any": 0, "back_all_zero": 0, "back_int_max": 0, "back_minus_two": -1,
    "back_int_min": -1, "back_of_a_later_calls_first_row": -1, "back_of_row_0_minus_two": -1, "null_penalty": -1, "penalty_nan": -1,
    "penalty_inf": -1, "penalty_negative": -1, "penalty_neg_zero": 0, "penalty_of_a_later_calls_first_row": -1,
    "penalty_of_row_0_is_ignored": 0, "negative_penalty_of_row_0_is_ignored": 0, "penalty_of_row_1": -1, "workspace_exact": 0,
    "workspace_short": -4, "workspace_of_the_plain_pass": -4, "workspace_misaligned": -2, "workspace_misaligned_and_short": -2,
    "bad_back_before_workspace": -1, "bad_penalty_before_alignment": -1}


def test_stage_track_ordered_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = dict(l.split() for l in lines[:len(EXPECTED_RC)])
    assert {k: int(v) for k, v in got.items()} == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    # one set of partial records, then four arrays of one entry per work item (8, 4, 8 and 4 bytes), each padded to 256 bytes
    assert rest[0] == "bytes 1280 1280 21248 0 0 0"
    assert rest[1] == "reach_back 5 9 9 2147483646 9 9"
    assert rest[2] == "facts_one rc=0 per=2 items=1 grid=1 set=256 offsets=(256,512,768,1024) bytes=1280"
    assert rest[3] == "facts_513 rc=0 per=2 items=2 grid=2 set=256 offsets=(256,512,768,1024) bytes=1280"
    assert rest[4] == "facts_240001 rc=0 per=2 items=469 grid=469 set=9472 offsets=(9472,13312,15360,19200) bytes=21248"
    assert rest[5] == "facts_2880001 rc=0 per=8 items=1407 grid=1407 set=28160 offsets=(28160,39424,45056,56320) bytes=61952"
    # 2^20 items of 2048: 24 bytes each behind a set of 2048 partial records
    assert rest[6] == "facts_int32_max rc=0 per=8 items=1048576 grid=2048 set=40960 offsets=(40960,8429568,12623872,21012480) " \
        "bytes=%d" % (40960 + 24 * 2 ** 20)
    assert len(rest) == 7


def _run_check(check, tmp_path, method, mu, n, curves, rows, reach, back, lams):
    rt = np.array(rows, dtype=_native.JOINT_ROW_DTYPE)
    paths = [os.path.join(str(tmp_path), name) for name in ("curves", "rows", "reach", "back", "penalty", "out")]
    curves.tofile(paths[0])
    rt.tofile(paths[1])
    np.array(reach, np.int32).tofile(paths[2])
    np.array(back, np.int32).tofile(paths[3])
    np.array(lams, np.float64).tofile(paths[4])
    subprocess.check_call([check, "pass", method.split("_")[0], float(mu).hex(), str(n)] + paths)
    raw = np.fromfile(paths[5], np.uint8)
    E = len(rows)
    take = lambda a, b, dtype: raw[a:b].copy().view(dtype)
    shifts, row_arg, own_idx = (take(4 * E * k, 4 * E * (k + 1), np.int32) for k in range(3))
    own_val = take(12 * E, 16 * E, np.uint32)
    row_min = take(16 * E, 24 * E, np.uint64)
    at = 24 * E
    last = take(at, at + 8 * n, np.uint64)
    moves = take(at + 8 * n, at + 8 * n + 2 * E * n, np.int16).reshape(E, n)
    origin = take(at + 8 * n + 2 * E * n, at + 8 * n + 6 * E * n, np.int32).reshape(E, n)
    assert raw.shape[0] == at + 8 * n + 6 * E * n
    return shifts, row_arg, own_idx, own_val, row_min, last, moves, origin


def _compare_with_host(got, rows, weights, lams, mu, reach, back, method):
    shifts, row_arg, own_idx, own_val, row_min, last, moves, origin = got
    kept = []
    want = track.track_ordered_host(rows, weights, lams, mu, reach, back, method, _keep=kept)
    assert shifts.tolist() == want.shifts.tolist() and row_arg.tolist() == want.row_arg.tolist()
    assert own_idx.tolist() == want.row_own_index.tolist() and (own_val == _bits(want.row_own_scores)).all()
    assert (row_min == _bits64(want.row_min)).all() and (last == _bits64(kept[-1])).all()
    assert (moves == want.moves).all() and (origin == want.prefix_arg).all()
    return want


@pytest.mark.parametrize("method", METHODS)
def test_the_header_on_the_cpu_equals_track_ordered_host(check, tmp_path, method):
    """track_core.hpp's candidates and track_step with order_jump and order_reach_back, the combine rule grouped another way than
    the kernels group it, and order_backtrack, run by a program of its own over the sequences of the GPU test but the longest, with
    backs 0, 1, 255, 256, n - 1, n + 7 and no limit and penalties that vary by row."""
    jumped = False
    for E, n, reach in cases.SHAPES[:-1] + [(4, 1025, 600), (3, 5, 1024)]:
        curves, rows, weights, lams, rs, mu, back = cases.sequence(E, n, reach, method, seed=3)
        lams[0] = 0.0                                       # (the program reads the table as the entry point does: row 0's is not read)
        want = _compare_with_host(_run_check(check, tmp_path, method, mu, n, curves, rows, rs, back, lams),
                                  track_cases.rows_of(curves, rows, n), weights, lams, mu, rs, back, method)
        jumped |= any(int(want.moves[e, want.shifts[e]]) == JUMP for e in range(1, E))
    assert jumped


def test_the_header_on_the_cpu_on_cases_written_here(check, tmp_path):
    for method in METHODS:
        for at in (256, 512):
            a, b = cases.prefix_tie_rows(1024, at, method)
            curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b])
            rows = [(1, 1.0), (1027, 1.0)]
            want = _compare_with_host(_run_check(check, tmp_path, method, 0.0, 1024, curves, rows, [0, 0], [ANY, 0], [0.0, 0.0625]),
                                      [a, b], [1.0, 1.0], [0.0, 0.0625], 0.0, [0, 0], [ANY, 0], method)
            assert want.prefix_arg[0, at] == at - 1
    # -0.0 through P under ccoeff with weight 0; back 0 at the last index; a penalty of 0; the move / jump tie
    curves = np.array([0.5, -0.5, -0.5, -0.25, -0.25, -0.25, 0.5, 0.125, 0.75, 0.25, 0.5, 0.5, 0.5, 0.0, 0.25, 0.5, 1.0, 0.75, 0.75, 0.0],
                      np.float32)
    for method in METHODS:
        for rows, n, mu, reach, back, lams in (([(0, 0.0), (3, 0.0)], 3, 0.0, [0, 0], [ANY, ANY], [0.0, 0.0]),
                                               ([(0, 0.0), (3, 1.0)], 3, 0.0, [0, 0], [ANY, 1], [0.0, 0.0]),
                                               ([(6, 1.0), (10, 1.0)], 4, 0.0, [0, 0], [ANY, 0], [0.0, 0.0625]),
                                               ([(6, 1.0), (10, 1.0), (7, 0.5)], 4, 0.125, [0, 1, 1], [ANY, 0, 2], [0.0, 0.0, 0.25]),
                                               ([(14, 1.0), (17, 1.0)], 3, 0.25, [0, 1], [ANY, 0], [0.0, 0.5])):
            got = _run_check(check, tmp_path, method, mu, n, curves, rows, reach, back, lams)
            _compare_with_host(got, track_cases.rows_of(curves, rows, n), [w for _o, w in rows], lams, mu, reach, back, method)


# ---------------------------------------------------------------------------------------------- the entry points, no GPU
def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    assert {"sushi_hip_track_order_bytes", "sushi_hip_track_forward_ordered", "sushi_hip_track_backtrack_ordered"} <= \
        set(_native.declared_symbols())
    assert _native.TRACK_BACK_ANY == -1 and track.BACK_ANY == -1
    assert L.sushi_hip_track_order_bytes(1, 1) == 1280 and L.sushi_hip_track_order_bytes(200, 240001) == 21248
    assert L.sushi_hip_track_order_bytes(0, 5) == 0 and L.sushi_hip_track_order_bytes(5, 0) == 0
    rows = np.array([(0, 1.0), (501, 0.0), (333, 2.5)], dtype=_native.JOINT_ROW_DTYPE)
    reach = np.array([0, 1024, 17], np.int32)
    back = np.array([0, -1, 600], np.int32)
    lams = np.array([0.5, 0.0, 2.0], np.float64)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)
    ptr = lambda a: None if a is None else a.ctypes.data

    def call(curves=P, n_curve=1000, rows=rows, reach=reach, back=back, lams=lams, n_rows=3, n_shift=499, method=0, step_cost=1e-3,
             row0=2, n_total=7, outs=(P,) * 9, mem=P, mem_bytes=1 << 16):
        return L.sushi_hip_track_forward_ordered(curves, n_curve, ptr(rows), ptr(reach), ptr(back), n_rows, n_shift, method, ptr(lams),
                                                 step_cost, row0, n_total, *outs, mem, mem_bytes, None)

    EINVAL, EALIGN = -1, -2
    assert call(mem_bytes=16) == _native.ENOSPACE                          # everything but the workspace is in order
    for name in ("curves", "rows", "reach", "back", "lams", "mem"):
        assert call(**{name: None}) == EINVAL, name
    for k in range(9):
        assert call(outs=tuple(None if i == k else P for i in range(9))) == EINVAL
    assert call(method=2) == EINVAL and call(n_rows=0) == EINVAL and call(n_shift=0) == EINVAL and call(n_shift=1001) == EINVAL
    assert call(row0=-1) == EINVAL and call(row0=5) == EINVAL and call(n_total=0) == EINVAL
    for bad in (np.nan, np.inf, -1e-300):
        assert call(step_cost=bad) == EINVAL
        for at in range(3):
            p = lams.copy()
            p[at] = bad
            assert call(lams=p) == EINVAL, (at, bad)
    p = lams.copy()
    p[0] = np.nan
    assert call(lams=p, row0=0, mem_bytes=16) == _native.ENOSPACE          # the sequence's row 0: its penalty is ignored
    for at, value in ((0, -2), (1, -2), (2, -(2 ** 31))):
        b = back.copy()
        b[at] = value
        assert call(back=b) == EINVAL, (at, value)
    b = back.copy()
    b[1] = 2 ** 31 - 1
    assert call(back=b, mem_bytes=16) == _native.ENOSPACE
    r = reach.copy()
    r[1] = 1025
    assert call(reach=r) == EINVAL
    bad = rows.copy()
    bad["curve_off"][1] = 502
    assert call(rows=bad) == EINVAL
    assert call(mem=odd(128)) == EALIGN and call(mem_bytes=1279) == _native.ENOSPACE
    assert call(curves=odd(2)) == EALIGN
    # D, moves, P, from, back, row_min, row_arg, row_own_index, row_own_score
    for k, off in enumerate((4, 1, 4, 2, 2, 4, 2, 2, 2)):
        assert call(outs=tuple(odd(off) if i == k else P for i in range(9))) == EALIGN, k

    def walk(moves=P, origin=P, back=P, row_arg=P, n_total=7, n_shift=499, out=P):
        return L.sushi_hip_track_backtrack_ordered(moves, origin, back, row_arg, n_total, n_shift, out, None)

    for name in ("moves", "origin", "back", "row_arg", "out"):
        assert walk(**{name: None}) == EINVAL, name
    assert walk(n_total=0) == EINVAL and walk(n_shift=0) == EINVAL
    assert walk(moves=odd(1)) == EALIGN
    for name in ("origin", "back", "row_arg", "out"):
        assert walk(**{name: odd(2)}) == EALIGN, name
