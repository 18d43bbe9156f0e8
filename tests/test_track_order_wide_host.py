"""Wide ordered tracking without a GPU: track_ordered_host(wide=True) against a loop restatement written here
(candidates in the order 0, -1, +1, ..., the jump from a prefix minimum), value bits, move words, prefix_arg and shifts;
track_ordered_margins_host(wide=True) against the minimum over all ordered paths on a padded axis, against wide=False where no
reach passes 1024 and against track_margins_host(wide=True) where no back binds; a mixed sequence; every new refusal, in Python and
in the library's host-only staging; the old refusals; ordered_wide_state_bytes; the kernels' arithmetic divided as they divide it,
compiled for the CPU (tests/host_track_order_wide_check.cpp, a program of its own under AddressSanitizer + UBSan); the scenario
that needs both extensions on the CPU oracle's rows."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import track_order_cases as ocases
import track_order_wide_cases as cases
import track_wide_cases as wcases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, track
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP, ANY = -32768, -1


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same(a, b):
    for name, x, y in zip(a._fields, a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("track_order_wide_check")), "host_track_order_wide_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_track_order_wide_check.cpp"), "-o", exe])
    return exe


# ---------------------------------------------------------------------------------------------- the forward pass, by a loop
def _loop_pass(rows, weights, lams, mu, reach, back, method):
    """The ordered recurrence by loops: per row the candidates 0, -1, +1, -2, +2, ... with strict replacement, the prefix minimum
    and its first index one element after the other, the jump read at min(j + back, n - 1) -> (D rows, moves, A rows, shifts)."""
    n = rows[0].shape[0]
    Ds, moves, As = [], [np.zeros(n, np.int16)], []
    for e, r in enumerate(rows):
        u = weights[e] * (-r.astype(np.float64) if method == "ccoeff_normed" else r.astype(np.float64))
        if e == 0:
            D = u
        else:
            X, near, nd = Ds[-1], Ds[-1].copy(), np.zeros(n, np.int64)
            for a in range(1, min(reach[e], n - 1) + 1):
                for d in (-a, a):
                    j = np.arange(max(0, -d), min(n, n - d))
                    cand = X[j + d] + mu * float(a)
                    take = cand < near[j]
                    near[j[take]], nd[j[take]] = cand[take], d
            t = np.full(n, n - 1) if back[e] < 0 else np.minimum(np.arange(n) + back[e], n - 1)
            jump = P[t] + lams[e]
            D = u + np.where(near <= jump, near, jump)
            moves.append(np.where(near <= jump, nd, JUMP).astype(np.int16))
        P, A, at = np.empty(n), np.empty(n, np.int32), 0
        for j in range(n):
            if D[j] < D[at]:
                at = j
            P[j], A[j] = D[at], at
        Ds.append(D)
        As.append(A)
    s = int(As[-1][n - 1])
    shifts = [s]
    for e in range(len(rows) - 1, 0, -1):
        m = int(moves[e][s])
        s = int(As[e - 1][n - 1 if back[e] < 0 else min(s + back[e], n - 1)]) if m == JUMP else s + m
        shifts.append(s)
    return Ds, moves, As, shifts[::-1]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [1026, 2053, 4104])
def test_the_wide_ordered_pass_is_the_loop(n, method):
    """n in {1026, 2053, 4104} x reach in {1025, 2048, 32767} x mu in {+0.0, -0.0}: eight rows, every kind of planted tie
    (track_wide_cases.sequence), track_order_cases' backs and penalties: every D's bits, every move word, prefix_arg, the shifts."""
    E = 9
    seen_wide = False
    for reach in (1025, 2048, 32767):
        for mu in (0.0, -0.0):
            curves, rows, weights, lams, rs, back, _g = cases.sequence(E, n, reach, method, seed=5)
            assert back == ocases.backs(E, n) and lams[1:] == ocases.penalties(E, cases.LAM)[1:]
            rr = cases.rows_of(curves, rows, n)
            kept = []
            got = track.track_ordered_host(rr, weights, lams, mu, rs, back, method, _keep=kept, wide=True)
            Ds, moves, As, shifts = _loop_pass(rr, weights, lams, mu, rs, back, method)
            for e in range(E):
                assert (_bits64(kept[e]) == _bits64(Ds[e])).all(), (reach, mu, e)
                assert (got.moves[e] == moves[e]).all() and (got.prefix_arg[e] == As[e]).all(), (reach, mu, e)
            assert got.shifts.tolist() == shifts
            seen_wide |= bool(((got.moves != JUMP) & (np.abs(got.moves.astype(np.int32)) > 1024)).any())
    assert seen_wide or n == 1026            # (on 1026 shifts only the move 0 <-> 1025 is wider than 1024)


# ---------------------------------------------------------------------------------------------- the margins
def _cheapest(c, a, b, r, lam, back):
    """test_track_order_margins_host.py's step from shift a of one event to shift b of the next, free moves."""
    choices = []
    if back < 0 or b >= a - back:
        choices.append(c + lam)
    if abs(a - b) <= r:
        choices.append(c)
    return min(choices) if choices else float("inf")


def _through(rows, weights, lams, reach, back, method, path, e):
    u = lambda i: float(weights[i]) * (-float(rows[i][path[i]]) if method == "ccoeff_normed" else float(rows[i][path[i]]))
    E = len(rows)
    p = u(0)
    for i in range(1, e + 1):
        p = u(i) + _cheapest(p, path[i - 1], path[i], reach[i], lams[i], back[i])
    if e == E - 1:
        return p
    c = u(E - 1)
    for i in range(E - 2, e, -1):
        c = u(i) + _cheapest(c, path[i], path[i + 1], reach[i + 1], lams[i + 1], back[i + 1])
    return p + _cheapest(c, path[e], path[e + 1], reach[e + 1], lams[e + 1], back[e + 1])


@pytest.mark.parametrize("method", METHODS)
def test_every_wide_marginal_is_the_minimum_over_all_ordered_paths(method):
    """n = 1100, E = 3, dyadic values, test_track_wide_host.py's padded axis: every row is high outside a few live shifts that lie
    so far apart that a reach above 1024 is what connects them; backs 0, 30, no limit, 1040, 0 and n by turns, penalties 1/8, 1/16, 1/4 and 0.  Every min-marginal at a live
    shift is exactly the minimum over all paths through the live shifts whose jumps obey the backs; some back binds, and some
    chosen move is wider than 1024."""
    rng = np.random.default_rng(8)
    n, E = 1100, 3
    sign = -1.0 if method == "ccoeff_normed" else 1.0
    live = [0, 3, 20, 1030, 1060, 1099]
    seen_wide = seen_bound = False
    for trial in range(8):
        rows = []
        for _e in range(E):
            r = np.full(n, sign * 1.0, np.float32)
            r[live] = (sign * rng.integers(0, 9, len(live)) / 16.0).astype(np.float32)
            rows.append(r)
        weights = [(1.0, 0.5, 2.0)[int(k)] for k in rng.integers(0, 3, E)]
        lams = [0.0] + [(0.125, 0.0625, 0.25, 0.0)[(trial + e) % 4] for e in range(1, E)]
        reach = [0, (1025, 1040, 1098, 1026, 32767, 1056, 1025, 1030)[trial], (1050, 1025, 1030, 5000, 1027, 1029, 1025, 1040)[trial]]
        back = [ANY] + [(0, 30, ANY, 1040, 0, n)[(trial + e) % 6] for e in range(1, E)]
        got = track.track_ordered_margins_host(rows, weights, lams, 0.0, reach, back, 0, method, wide=True)
        paths = list(itertools.product(live, repeat=E))
        for e in range(E):
            costs = [_through(rows, weights, lams, reach, back, method, p, e) for p in paths]
            for j in live:
                assert got.marginals[e, j] == min(c for c, p in zip(costs, paths) if p[e] == j), (trial, e, j)
        assert got.cost == got.marginals[E - 1].min() and set(got.shifts.tolist()) <= set(live)
        free = track.track_ordered_margins_host(rows, weights, lams, 0.0, reach, ANY, 0, method, wide=True)
        seen_bound |= bool((free.marginals < got.marginals).any())
        seen_wide |= any(w != JUMP and abs(w) > 1024 for w in (int(got.moves[e, got.shifts[e]]) for e in range(1, E)))
    assert seen_wide and seen_bound


@pytest.mark.parametrize("method", METHODS)
def test_wide_is_the_ordered_pass_where_no_reach_passes_1024(method):
    E, n = 6, 1500
    curves, rows, weights, lams, _rs, back, guard = cases.sequence(E, n, 0, method, seed=1)
    rr = cases.rows_of(curves, rows, n)
    for mu, reach in ((0.0, [0, 1024, 3, 0, 700, 1024]), (2.0 ** -12, 1024), (1e-3, [5000, 64, 64, 64, 64, 64])):
        a = track.track_ordered_margins_host(rr, weights, lams, mu, reach, back, guard, method)
        b = track.track_ordered_margins_host(rr, weights, lams, mu, reach, back, guard, method, wide=True)
        _same(a, b)
        _same(track.track_ordered_host(rr, weights, lams, mu, reach, back, method),
              track.track_ordered_host(rr, weights, lams, mu, reach, back, method, wide=True))


@pytest.mark.parametrize("method", METHODS)
def test_without_a_limit_it_is_the_plain_wide_pass(method):
    """Every back without a limit (or >= n - 1) and one penalty: every field the two share equals track_margins_host(wide=True)'s."""
    E, n = 5, 4104
    curves, rows, weights, _lams, _rs, _back, guard = cases.sequence(E, n, 0, method, seed=9)
    rr = cases.rows_of(curves, rows, n)
    for back in (ANY, [ANY, n - 1, n + 7, ANY, 2 ** 31 - 1]):
        for mu in (0.0, -0.0):
            a = track.track_margins_host(rr, weights, cases.LAM, mu, cases.MIXED_REACH, guard, method, wide=True)
            b = track.track_ordered_margins_host(rr, weights, cases.LAM, mu, cases.MIXED_REACH, back, guard, method, wide=True)
            for name in a._fields:
                x, y = np.asarray(getattr(a, name)), np.asarray(getattr(b, name))
                assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), name


@pytest.mark.parametrize("method", METHODS)
def test_a_mixed_sequence(method):
    """Reaches [0, 7, 1025, 64, 3000]: the wide rows' window minima are _near_wide's, the others' the loop's -- the whole pass and
    its margins against one that takes the loop in every row."""
    E, n = 5, 4104
    curves, rows, weights, lams, rs, back, guard = cases.sequence(E, n, cases.MIXED_REACH, method, seed=9)
    assert rs == cases.MIXED_REACH
    rr = cases.rows_of(curves, rows, n)
    got = track.track_ordered_margins_host(rr, weights, lams, -0.0, rs, back, guard, method, wide=True)
    wide_form = track._near_wide
    track._near_wide = track._near                   # (the loop has no bound of its own)
    try:
        want = track.track_ordered_margins_host(rr, weights, lams, -0.0, rs, back, guard, method, wide=True)
    finally:
        track._near_wide = wide_form
    _same(got, want)
    Ds, moves, As, shifts = _loop_pass(rr, weights, lams, -0.0, rs, back, method)
    assert got.shifts.tolist() == shifts and (_bits64(got.D) == _bits64(np.stack(Ds))).all()


# ---------------------------------------------------------------------------------------------- refusals
def test_python_refusals():
    r = np.zeros(1100, np.float32)
    for call in (lambda **kw: track.track_ordered_host([r, r, r], [1.0] * 3, 0.5, kw.pop("mu", 0.0), kw.pop("reach"), ANY, **kw),
                 lambda **kw: track.track_ordered_margins_host([r, r, r], [1.0] * 3, 0.5, kw.pop("mu", 0.0), kw.pop("reach"), ANY, 0, **kw)):
        with pytest.raises(SushiError) as e:
            call(reach=[0, 5, 1025])                                                                # wide=False: as before
        assert "event 2" in str(e.value) and "1025" in str(e.value) and "1024" in str(e.value)
        with pytest.raises(SushiError) as e:
            call(reach=[0, 32768, 5], wide=True)
        assert "event 1" in str(e.value) and "32768" in str(e.value) and "32767" in str(e.value)
        with pytest.raises(SushiError) as e:
            call(reach=[0, 5, 1025], mu=0.25, wide=True)
        assert "event 2" in str(e.value) and "1025" in str(e.value) and "0.25" in str(e.value) and "penalty" in str(e.value)
        assert call(reach=[0, 5, 1024], mu=0.25, wide=True).shifts.tolist() == [0, 0, 0]
        assert call(reach=[9999, 5, 32767], wide=True).shifts.tolist() == [0, 0, 0]


def test_ordered_wide_state_bytes():
    records = track.wide_workspace_bytes(24001)
    assert records == 2 * 192256 + 2 * 96256
    plain = 4 * 24001 * 6 + 3 * 24001 * 8
    kept = 4 * 24001 * 14 + 4 * 24001 * 8
    assert track.ordered_wide_state_bytes(4, 24001) == plain + records
    assert track.ordered_wide_state_bytes(4, 24001, margins=True) == kept + records
    assert track.ordered_wide_state_bytes(4, 24001, margins=True, marginals=True) == kept + 4 * 24001 * 8 + records
    assert track.ordered_wide_state_bytes(4, 24001, marginals=True) == plain + records            # marginals belong to margins


def test_find_ordered_wide_track_refuses_on_the_host():
    from test_track_host import _NoDevice
    stream = _NoDevice()
    patterns = [np.zeros((1, 6000), np.uint8)] * 4
    centres = [1.0, 2.0, 3.0, 20.0]
    find = track.find_ordered_wide_track
    # 17 s between events 2 and 3 at 6e-3: a reach of 1225 -- accepted here (the call then fails at the device), refused beside a step cost
    with pytest.raises(SushiError) as e:
        find(stream, patterns, centres, 1.0, 0.5, order=True, max_rate=6e-3, step_cost=1e-4)
    assert "event 3" in str(e.value) and "1225" in str(e.value) and "0.0001" in str(e.value)
    with pytest.raises(SushiError) as e:
        find(stream, patterns, centres, 1.0, 0.5, order=True, max_rate=0.2)
    assert "event 3" in str(e.value) and "40801" in str(e.value) and "32767" in str(e.value)
    for kw, need in ((dict(), track.ordered_wide_state_bytes(4, 24001)),
                     (dict(margins=True), track.ordered_wide_state_bytes(4, 24001, margins=True)),
                     (dict(margins=True, marginals=True), track.ordered_wide_state_bytes(4, 24001, margins=True, marginals=True))):
        with pytest.raises(SushiError) as e:
            find(stream, patterns, centres, 1.0, [0.0, 0.5, 0.25, 0.5], order=True, max_rate=6e-3, max_state_bytes=need - 1, **kw)
        assert str(need) in str(e.value) and "window records" in str(e.value) and "find_ordered_wide_track" in str(e.value)
    for kw in (dict(guard=5), dict(marginals=True)):
        with pytest.raises(SushiError) as e:
            find(stream, patterns, centres, 1.0, 0.5, max_rate=6e-3, **kw)
        assert "margins=True" in str(e.value)
    for bad in (dict(), dict(reach=1, max_rate=1e-3)):
        with pytest.raises(SushiError):
            find(stream, patterns, centres, 1.0, 0.5, **bad)
    for bad in (dict(order=[0, 0, 0]), dict(order="yes"), dict(penalty=[0.5] * 3), dict(penalty=[0.0, 0.5, -0.5, 0.5])):
        args = dict(penalty=0.5, reach=2000)
        args.update(bad)
        with pytest.raises(SushiError):
            find(stream, patterns, centres, 1.0, **args)
    with pytest.raises(TypeError):
        find(stream, patterns, centres, 1.0, 0.5, reach=2000, wide=True)       # the arguments are find_ordered_track's, minus wide


def test_the_old_refusals_still_refuse():
    """Called as tests/test_track_wide_host.py calls them."""
    from test_track_host import _NoDevice
    stream = _NoDevice()
    patterns = [np.zeros((1, 6000), np.uint8)] * 4
    centres = [1.0, 2.0, 3.0, 20.0]
    for kw in (dict(order=True), dict(order=[None, 5, 5, 5])):
        with pytest.raises(SushiError) as e:
            track.find_track(stream, patterns, centres, 1.0, 0.5, max_rate=6e-3, wide=True, **kw)
        assert "ordered pass" in str(e.value) and "1024" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, [0.5] * 4, max_rate=6e-3, wide=True)
    assert "ordered pass" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.find_ordered_track(stream, patterns, centres, 1.0, 0.5, max_rate=1e-3, wide=True)
    assert "ordered pass" in str(e.value) and "1024" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.find_ordered_track(stream, patterns, centres, 1.0, 0.5, order=True, max_rate=6e-3)
    assert "event 3" in str(e.value) and "1225" in str(e.value) and "1024" in str(e.value)
    with pytest.raises(SushiError):
        track.TrackState.nbytes(4, 24001, ordered=True, wide=True)
    with pytest.raises(SushiError) as e:
        track.TrackState(3, 8, None, ordered=True, wide=True)
    assert "ordered pass" in str(e.value)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """The library's host-only staging: no launch is made, so no GPU is needed."""
    L = _native.lib()
    names = {"sushi_hip_track_order_wide_bytes", "sushi_hip_track_order_margins_wide_bytes", "sushi_hip_track_forward_ordered_wide",
             "sushi_hip_track_forward_ordered_wide_keep", "sushi_hip_track_order_margins_wide"}
    assert names <= set(_native.declared_symbols()) and L.sushi_hip_abi_version() == 13
    for n in (1, 499, 240001):
        records = track.wide_workspace_bytes(n)
        assert L.sushi_hip_track_order_wide_bytes(3, n) == L.sushi_hip_track_order_bytes(3, n) + records
        assert L.sushi_hip_track_order_margins_wide_bytes(3, n) == L.sushi_hip_track_order_margins_bytes(3, n) + records
    for bad in ((0, 5), (5, 0), (-1, -1)):
        assert L.sushi_hip_track_order_wide_bytes(*bad) == 0 and L.sushi_hip_track_order_margins_wide_bytes(*bad) == 0
    rows = np.array([(0, 1.0), (501, 0.0), (333, 2.5)], dtype=_native.JOINT_ROW_DTYPE)
    reach = np.array([0, 32767, 1025, 2000], np.int32)
    back = np.array([0, -1, 600, 3], np.int32)
    lams = np.array([0.5, 0.0, 2.0, 0.25], np.float64)
    guard = np.array([0, 120, 5], np.int32)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first
    odd = ctypes.c_void_p((1 << 20) + 128)
    ptr = lambda a: None if a is None else a.ctypes.data
    EINVAL, EALIGN, ENOSPACE = -1, -2, _native.ENOSPACE

    def forward(fn, reach=reach, back=back, lams=lams, step_cost=0.0, row0=2, mem=P, mem_bytes=16, D=P):
        return fn(P, 1000, ptr(rows), ptr(reach), ptr(back), 3, 499, 0, ptr(lams), step_cost, row0, 7, D, P, P, P, P, P, P, P, P, mem,
                  mem_bytes, None)

    def margins(fn, reach=reach, back=back, lams=lams, step_cost=0.0, row0=2, mem=P, mem_bytes=16, D=P):
        return fn(P, 1000, ptr(rows), ptr(reach), ptr(back), ptr(guard), 3, 499, 0, ptr(lams), step_cost, row0, 7, D, P, P, P, P, P, P,
                  P, P, P, None, mem, mem_bytes, None)

    def changed(a, at, value):
        a = a.copy()
        a[at] = value
        return a

    for call, fns, plain_bytes in ((forward, (L.sushi_hip_track_forward_ordered_wide, L.sushi_hip_track_forward_ordered_wide_keep),
                                    L.sushi_hip_track_order_bytes(3, 499)),
                                   (margins, (L.sushi_hip_track_order_margins_wide,), L.sushi_hip_track_order_margins_bytes(3, 499))):
        for fn in fns:
            assert call(fn) == ENOSPACE                                          # good arguments: the workspace is what fails
            assert call(fn, step_cost=-0.0) == ENOSPACE
            assert call(fn, reach=changed(reach, 1, 32768)) == EINVAL            # reach 32768, before the workspace ...
            assert call(fn, reach=changed(reach, 1, 32768), mem=odd) == EINVAL   # ... and before its alignment
            assert call(fn, reach=changed(reach, 2, -1)) == EINVAL
            assert call(fn, step_cost=1e-3) == EINVAL                            # reach 1025 with mu != 0
            assert call(fn, step_cost=1e-3, mem=odd) == EINVAL
            assert call(fn, reach=np.array([0, 1024, 7, 1024], np.int32), step_cost=1e-3) == ENOSPACE
            assert call(fn, mem=odd) == EALIGN                                   # a misaligned workspace
            assert call(fn, mem_bytes=plain_bytes) == ENOSPACE                   # the ordered call's workspace is too short
            assert call(fn, mem=None) == EINVAL
            for name in ("reach", "back", "lams"):                               # null tables
                assert call(fn, **{name: None}) == EINVAL, name
            assert call(fn, back=changed(back, 1, -2)) == EINVAL and call(fn, lams=changed(lams, 2, np.nan)) == EINVAL
            assert call(fn, D=ctypes.c_void_p((1 << 20) + 4), mem_bytes=1 << 30) == EALIGN
    # reach[0]: used by a forward call that continues a sequence, ignored in the sequence's row 0, never used by a margins call
    assert forward(L.sushi_hip_track_forward_ordered_wide, reach=changed(reach, 0, 32768)) == EINVAL
    assert forward(L.sushi_hip_track_forward_ordered_wide, reach=changed(reach, 0, 32768), row0=0) == ENOSPACE
    assert margins(L.sushi_hip_track_order_margins_wide, reach=changed(reach, 0, 32768)) == ENOSPACE
    # reach[3]: the row after a margins call that ends below the sequence's last row
    assert margins(L.sushi_hip_track_order_margins_wide, reach=changed(reach, 3, 32768)) == EINVAL
    assert margins(L.sushi_hip_track_order_margins_wide, reach=changed(reach, 3, 32768), row0=4) == ENOSPACE
    # the ordered entry points keep their bound
    for fn in (L.sushi_hip_track_forward_ordered, L.sushi_hip_track_forward_ordered_keep):
        assert forward(fn, reach=changed(reach, 1, 1025)) == EINVAL
        assert forward(fn, reach=np.array([0, 1024, 7, 0], np.int32)) == ENOSPACE
    assert margins(L.sushi_hip_track_order_margins, reach=changed(reach, 1, 1025)) == EINVAL


# ---------------------------------------------------------------------------------------------- the kernels' arithmetic on the CPU
EXPECTED_RC = {   # case of host_track_order_wide_check validate -> what stage_track_ordered_wide and stage_order_margins_wide return
    "good": (0, 0), "step_cost_neg_zero": (0, 0), "narrow_reaches_with_step_cost": (0, 0), "reach_32768": (-1, -1),
    "reach_negative": (-1, -1), "wide_reach_with_step_cost": (-1, -1), "reach_1025_with_step_cost": (-1, -1),
    "first_reach_32768": (-1, 0), "reach_of_row_0_is_ignored": (0, 0), "reach_after_the_call_32768": (0, -1),
    "reach_after_the_sequence_is_ignored": (0, 0), "null_reach": (-1, -1), "null_back": (-1, -1), "null_penalty": (-1, -1),
    "back_minus_two": (-1, -1), "penalty_nan": (-1, -1), "step_cost_negative": (-1, -1), "reach_32768_before_workspace": (-1, -1),
    "wide_reach_with_step_cost_before_alignment": (-1, -1), "bad_back_before_workspace": (-1, -1),
    "workspace_misaligned_and_short": (-2, -2), "workspace_misaligned": (-2, -2), "null_mem": (-1, -1),
    # (three rows over 499 shifts: the forward layout is 1280 bytes before the records and the margins layout 1024, so the margins'
    # exact size, and the forward's less one byte, are short for the forward call alone)
    "workspace_exact_forward": (0, 0), "workspace_exact_margins": (-4, 0), "workspace_short": (-4, 0),
    "workspace_of_the_ordered_call": (-4, -4)}


def test_stage_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in lines[:len(EXPECTED_RC)]}
    assert got == EXPECTED_RC
    rec = track.wide_workspace_bytes
    L = _native.lib()
    assert lines[len(EXPECTED_RC)] == "bytes %d %d %d 0 0" % (1280 + rec(1), 1280 + rec(499), L.sushi_hip_track_order_bytes(200, 240001) + rec(240001))
    assert lines[len(EXPECTED_RC) + 1] == "margin_bytes %d %d %d 0 0" % (1024 + rec(1), 1024 + rec(499), 26624 + rec(240001))
    assert lines[len(EXPECTED_RC) + 2] == ("facts_499 rc=0 per=2 items=1 plain=1280 records=(1280,5376,9472,11520) bytes=13568 tile_grid=1 "
                                           "wide_rows=2")


def _by_check(check, tmp_path, method, mu, n, curves, rows, reach, back, lams):
    paths = [os.path.join(str(tmp_path), name) for name in ("curves", "rows", "reach", "back", "penalty", "out")]
    curves.tofile(paths[0])
    np.array(rows, dtype=_native.JOINT_ROW_DTYPE).tofile(paths[1])
    np.array(reach, np.int32).tofile(paths[2])
    np.array(back, np.int32).tofile(paths[3])
    np.array(lams, np.float64).tofile(paths[4])
    subprocess.check_call([check, "pass", method.split("_")[0], float(mu).hex(), str(n)] + paths)      # (exit status 4: a difference)
    return np.fromfile(paths[5], np.uint8)


@pytest.mark.parametrize("method", METHODS)
def test_the_divided_arithmetic_on_the_cpu_equals_the_host(check, tmp_path, method):
    """Work items, staged tiles, per-item records, scan and apply, forward and backward, under AddressSanitizer + UBSan: inside the
    program every window minimum against the candidate loop, here every output against track_ordered_margins_host(wide=True).  The
    mixed reaches on 4104 shifts (two work items of 2048 and a third of eight shifts), and the widest reach on 2053 shifts."""
    for n, reach, mu in ((4104, cases.MIXED_REACH, -0.0), (2053, 32767, 0.0), (1026, 1025, 0.0)):
        E = 5
        curves, rows, weights, lams, rs, back, _guard = cases.sequence(E, n, reach, method, seed=9)
        raw = _by_check(check, tmp_path, method, mu, n, curves, rows, rs, back, lams)
        want = track.track_ordered_margins_host(cases.rows_of(curves, rows, n), weights, lams, mu, rs, back, 0, method, wide=True)
        at = 0

        def take(dtype, count):
            nonlocal at
            out = raw[at:at + count * np.dtype(dtype).itemsize].view(dtype)
            at += out.nbytes
            return out

        assert take(np.int32, E).tolist() == want.shifts.tolist() and take(np.int32, E).tolist() == want.row_arg.tolist()
        assert (take(np.uint64, E) == _bits64(want.row_min)).all() and (take(np.uint64, E) == _bits64(want.c_min)).all()
        assert (take(np.int16, E * n).reshape(E, n) == want.moves).all()
        assert (take(np.int32, E * n).reshape(E, n) == want.prefix_arg).all()
        assert (take(np.uint64, E * n).reshape(E, n) == _bits64(want.D)).all()
        assert (take(np.uint64, E * n).reshape(E, n) == _bits64(want.marginals)).all() and at == raw.shape[0]


# ---------------------------------------------------------------------------------------------- the scenario on the oracle
@pytest.fixture(scope="module")
def scenario_rows(oracle):
    import segment_cases
    from sushi_amd import joint
    dst, src = cases.streams()
    patterns, _centres, bases = cases.scenario(dst, src)
    lens = [p.shape[1] for p in patterns]
    assert joint.joint_window(bases, lens, dst.data.shape[1], int(cases.RATE * cases.WINDOW)) == (cases.K_LO, cases.N_SHIFT)
    assert track.rate_reach(bases, cases.MAX_RATE, cases.SLACK) == cases.REACH
    assert track.order_back(bases, lens) == [ANY] + cases.BACK[1:]
    return segment_cases.oracle_rows(oracle, dst, patterns, bases, cases.K_LO, cases.N_SHIFT)


def _shifts_and_jumps(got):
    return (got.shifts + cases.K_LO).tolist(), [e for e in range(1, 10) if got.moves[e, got.shifts[e]] == JUMP]


def test_the_scenario_needs_order_and_a_wide_reach_at_once(oracle, scenario_rows):
    """tests/track_order_wide_cases.py's conditions (a) - (d) on the CPU oracle's rows."""
    rows, w = scenario_rows, [1.0] * 10
    back = [ANY] + cases.BACK[1:]
    assert [oracle.argmin_first(r) + cases.K_LO for r in rows] == cases.DECOYED_K         # a lone search takes both decoys
    assert cases.REACH[5] == 2399 and cases.TRUE_K[4] - cases.TRUE_K[5] == 1890
    for v, d in zip(cases.VICTIMS, cases.DECOYS):                                          # the jump a decoy needs is forbidden
        assert abs(d) > cases.BACK[v if d < 0 else v + 1]
    for lam in cases.PENALTIES:
        # (a)
        plain = track.track_host(rows, w, lam, 0.0, cases.REACH, wide=True)
        assert _shifts_and_jumps(plain) == (cases.DECOYED_K, cases.DECOYED_JUMPS), lam
        wide = track.track_ordered_host(rows, w, lam, 0.0, cases.REACH, back, wide=True)
        assert _shifts_and_jumps(wide) == (cases.TRUE_K, []), lam
        assert wide.moves[5, wide.shifts[5]] == 1890
        assert abs(plain.cost - cases.RESULTS[lam][0]) < 1e-12 and abs(wide.cost - cases.RESULTS[lam][1]) < 1e-12
        # (b)
        clipped = track.track_ordered_host(rows, w, lam, 0.0, cases.CLIPPED, back)
        assert _shifts_and_jumps(clipped) == (cases.TRUE_K, [5]), lam
        assert abs(clipped.cost - (wide.cost + lam)) < 1e-12
        # (c)
        with pytest.raises(SushiError) as e:
            track.track_ordered_host(rows, w, lam, 0.0, cases.REACH, back)
        assert "event 5" in str(e.value) and "2399" in str(e.value) and "1024" in str(e.value)
    # below the range the wide ordered pass goes wrong too, by two legal descents: no reach changes that
    small = track.track_ordered_host(rows, w, cases.PENALTY_TOO_SMALL, 0.0, cases.REACH, back, wide=True)
    assert _shifts_and_jumps(small) == (cases.DETOUR_K, [1, 2, 3])
    # (d)
    mo = track.track_ordered_margins_host(rows, w, cases.PENALTY, 0.0, cases.REACH, back, cases.GUARD, wide=True)
    mp = track.track_margins_host(rows, w, cases.PENALTY, 0.0, cases.REACH, cases.GUARD, wide=True)
    for v in cases.VICTIMS:
        ordered, plain = mo.alt[v] - mo.through[v], mp.alt[v] - mp.through[v]
        assert abs(ordered - cases.ORDERED_MARGINS[v]) < 5e-4 and abs(plain - cases.PLAIN_MARGINS[v]) < 5e-4
        assert ordered > 2 * plain and mo.alt_arg[v] + cases.K_LO == cases.ORDERED_ALT_K[v]
    for lam, margin in cases.DETOUR_MARGINS.items():
        m = track.track_ordered_margins_host(rows, w, lam, 0.0, cases.REACH, back, cases.GUARD, wide=True)
        assert abs(m.alt[1] - m.through[1] - margin) < 5e-4 and abs(m.alt[2] - m.through[2] - margin) < 5e-4
        assert m.alt_arg[1] + cases.K_LO == cases.DETOUR_K[1]
