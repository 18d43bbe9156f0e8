"""Wide tracking without a GPU: the O(n) window minimum (sushi_amd/track.py _near_wide) against the candidate loop
(_near), value bits and move words; track_host / track_margins_host with wide=True against a brute force over all paths on padded
axes, against wide=False where no reach passes 1024, and on a mixed sequence; every new refusal, in Python and in the library; the
kernels' own header compiled for the CPU (tests/host_track_wide_check.cpp, a program of its own under AddressSanitizer + UBSan);
the long-gap scenario on the CPU oracle's rows: what a clipped reach costs, and where it goes wrong."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import track_wide_cases as cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, track
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP = -32768


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("track_wide_check")), "host_track_wide_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_track_wide_check.cpp"), "-o", exe])
    return exe


# ---------------------------------------------------------------------------------------------- _near_wide
@pytest.mark.parametrize("n", cases.NS)
def test_near_wide_is_the_candidate_loop(n):
    """Every reach of cases.REACHES (below, equal to and above n - 1), both free moves, every kind of planted tie: the value's bits
    and the move word of every shift."""
    for kind in cases.KINDS:
        for sign in (1.0, -1.0):                      # the costs of 'sqdiff_normed' and of 'ccoeff_normed'
            D = cases.tie_row(n, kind, seed=3) * sign
            for reach in cases.REACHES:
                for mu in (0.0, -0.0):
                    want, want_d = track._near(D, reach, mu, moves=True)
                    got, got_d = track._near_wide(D, reach, mu, moves=True)
                    assert (_bits64(got) == _bits64(want)).all() and (got_d == want_d).all(), (kind, sign, reach, mu)
                    assert got_d.dtype == np.int16 and track._near_wide(D, reach, mu)[1] is None
    with pytest.raises(SushiError):
        track._near_wide(np.zeros(4), 2000, 1e-3)


def test_the_planted_ties_are_met():
    n = 5000
    both = cases.tie_row(9000, "both_sides", seed=3)                                              # minima at 2200 +- 1100, 4500 +- 1, 6800 +- 300
    near, d = track._near_wide(both, 1500, 0.0, moves=True)
    assert d[2200] == -1100 and d[4500] == -1 and d[6800] == -300                                 # equal minima at -a and +a: -a
    one = cases.tie_row(n, "one_side", seed=3)
    _near, d = track._near_wide(one, 1500, 0.0, moves=True)
    assert d[n // 2] == 5 and d[n // 2 + 6] == -1 and d[n // 2 + 7] == -2 and d[n // 2 + 8] == 1   # several on one side: the nearest
    own = cases.tie_row(n, "own", seed=3)
    _near, d = track._near_wide(own, 1500, 0.0, moves=True)
    assert d[n // 2] == 0 and d[0] == 0 and d[n - 1] == 0 and d[n // 2 + 1] == -1                 # an own value equal to the window's
    zeros = cases.tie_row(n, "zeros", seed=3)
    for mu, moved_bits in ((0.0, 0), (-0.0, 1 << 63)):
        near, d = track._near_wide(zeros, 1500, mu, moves=True)
        assert d[n // 2 - 4] == 0 and _bits64(near[n // 2 - 4]) == 1 << 63                        # -0.0 at d = 0 keeps its bits
        assert d[n // 2 - 5] == 1 and _bits64(near[n // 2 - 5]) == moved_bits                     # -0.0 at d = +1: + mu
        assert d[n // 2 + 3] == -1 and _bits64(near[n // 2 + 3]) == moved_bits
    const, d = track._near_wide(cases.tie_row(n, "constant"), 32767, 0.0, moves=True)
    assert not d.any() and (const == 0.625).all()


# ---------------------------------------------------------------------------------------------- track_host(wide=True)
def _path_cost(rows, weights, lam, reach, method, path):
    """test_track_host.py's in-order cost of a path, free moves."""
    u = lambda e: float(weights[e]) * (-float(rows[e][path[e]]) if method == "ccoeff_normed" else float(rows[e][path[e]]))
    c = u(0)
    for e in range(1, len(rows)):
        c = u(e) + (c if abs(path[e] - path[e - 1]) <= reach[e] else c + lam)
    return c


@pytest.mark.parametrize("method", METHODS)
def test_the_wide_pass_finds_the_minimum_over_all_paths(method):
    """n = 1100, E = 3, dyadic values: every row is high (1.0; -0.0 under ccoeff's sign would be low, so -1.0 there is 'high' for
    the cost -(-1) = 1) outside a live region of a few shifts spread so far apart that a reach above 1024 is what connects them.
    The pass's cost is the minimum over all paths through the live shifts (every other shift costs more in every row), exactly,
    and so is every min-marginal."""
    rng = np.random.default_rng(8)
    n, E = 1100, 3
    sign = -1.0 if method == "ccoeff_normed" else 1.0
    live = [0, 3, 20, 1030, 1060, 1099]
    seen_wide = False
    for trial in range(6):
        rows = []
        for _e in range(E):
            r = np.full(n, sign * 1.0, np.float32)
            r[live] = (sign * rng.integers(0, 9, len(live)) / 16.0).astype(np.float32)
            rows.append(r)
        weights = [(1.0, 0.5, 2.0)[int(k)] for k in rng.integers(0, 3, E)]
        lam = (0.125, 0.25, 0.5, 1.0, 0.0625, 2.0)[trial]
        reach = [0, (1025, 1040, 1098, 1099, 32767, 1056)[trial], (1050, 1025, 1030, 5000, 1027, 1099)[trial]]
        got = track.track_margins_host(rows, weights, lam, 0.0, reach, 0, method, wide=True)
        paths = list(itertools.product(live, repeat=E))
        costs = [_path_cost(rows, weights, lam, reach, method, p) for p in paths]
        assert got.cost == min(costs) and _path_cost(rows, weights, lam, reach, method, got.shifts.tolist()) == got.cost
        assert set(got.shifts.tolist()) <= set(live)
        for e in range(E):
            for j in live:
                assert got.marginals[e, j] == min(c for c, p in zip(costs, paths) if p[e] == j), (trial, e, j)
        words = [int(got.moves[e, got.shifts[e]]) for e in range(1, E)]
        seen_wide |= any(w != JUMP and abs(w) > 1024 for w in words)
    assert seen_wide


@pytest.mark.parametrize("method", METHODS)
def test_wide_is_the_plain_pass_where_no_reach_passes_1024(method):
    E, n = 6, 1500
    curves, rows, weights = cases.sequence(E, n, method, seed=1)
    rs = cases.rows_of(curves, rows, n)
    for mu, reach in ((0.0, [0, 1024, 3, 0, 700, 1024]), (2.0 ** -12, 1024), (1e-3, [5000, 64, 64, 64, 64, 64])):
        a = track.track_margins_host(rs, weights, 0.0625, mu, reach, [0, 120] * 3, method)
        b = track.track_margins_host(rs, weights, 0.0625, mu, reach, [0, 120] * 3, method, wide=True)
        for name, x, y in zip(a._fields, a, b):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name


@pytest.mark.parametrize("method", METHODS)
def test_a_mixed_sequence(method):
    """Reaches [0, 7, 1025, 64, 3000]: the wide rows' window minima are _near_wide's, the others' the loop's -- the whole pass
    against one that takes the loop in every row."""
    E, n = 5, 4104
    curves, rows, weights = cases.sequence(E, n, method, seed=9)
    rs = cases.rows_of(curves, rows, n)
    got = track.track_margins_host(rs, weights, 0.0625, -0.0, cases.MIXED_REACH, [0, 120, 7, 0, 5000], method, wide=True)
    wide_form = track._near_wide
    track._near_wide = track._near                   # (the loop has no bound of its own)
    try:
        want = track.track_margins_host(rs, weights, 0.0625, -0.0, cases.MIXED_REACH, [0, 120, 7, 0, 5000], method, wide=True)
    finally:
        track._near_wide = wide_form
    for name, x, y in zip(got._fields, got, want):
        assert np.asarray(x).tobytes() == np.asarray(y).tobytes(), name
    words = [int(got.moves[e, got.shifts[e]]) for e in range(1, E)]
    assert any(w != JUMP and abs(w) > 1024 for w in words)


# ---------------------------------------------------------------------------------------------- refusals
def test_python_refusals():
    r = np.zeros(1100, np.float32)
    assert track.WIDE_MAX_REACH == _native.TRACK_WIDE_MAX_REACH == 32767
    assert track.checked_reach([9, 32767], 2, first_row=4, wide=True).tolist() == [9, 32767]
    assert track.checked_reach([40000, 32767], 2, wide=True).tolist() == [0, 32767]               # row 0's is ignored
    with pytest.raises(SushiError) as e:
        track.checked_reach([9, 32768], 2, first_row=4, wide=True)
    assert "event 5" in str(e.value) and "32768" in str(e.value) and "32767" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.checked_reach([9, 1025], 2, first_row=4)
    assert "event 5" in str(e.value) and "1024" in str(e.value)
    for call in (lambda **kw: track.track_host([r, r, r], [1.0] * 3, 0.5, kw.pop("mu", 0.0), kw.pop("reach"), **kw),
                 lambda **kw: track.track_margins_host([r, r, r], [1.0] * 3, 0.5, kw.pop("mu", 0.0), kw.pop("reach"), 0, **kw)):
        with pytest.raises(SushiError) as e:
            call(reach=[0, 5, 1025])                                                                # wide=False: as before
        assert "event 2" in str(e.value) and "1025" in str(e.value) and "1024" in str(e.value)
        with pytest.raises(SushiError) as e:
            call(reach=[0, 32768, 5], wide=True)
        assert "event 1" in str(e.value) and "32768" in str(e.value)
        with pytest.raises(SushiError) as e:
            call(reach=[0, 5, 1025], mu=0.25, wide=True)
        assert "event 2" in str(e.value) and "1025" in str(e.value) and "0.25" in str(e.value) and "penalty" in str(e.value)
        assert call(reach=[0, 5, 1024], mu=0.25, wide=True).shifts.tolist() == [0, 0, 0]
        assert call(reach=[9999, 5, 32767], wide=True).shifts.tolist() == [0, 0, 0]
    need = track.TrackState.nbytes(4, 24001)
    assert track.wide_workspace_bytes(24001) == 2 * 192256 + 2 * 96256
    assert track.TrackState.nbytes(4, 24001, wide=True) == need + track.wide_workspace_bytes(24001)
    assert track.TrackState.nbytes(4, 24001, keep=True, marginals=True, wide=True) == \
        track.TrackState.nbytes(4, 24001, keep=True, marginals=True) + track.wide_workspace_bytes(24001)
    with pytest.raises(SushiError):
        track.TrackState.nbytes(4, 24001, ordered=True, wide=True)


def test_find_track_wide_refuses_on_the_host():
    from test_track_host import _NoDevice
    stream = _NoDevice()
    patterns = [np.zeros((1, 6000), np.uint8)] * 4
    centres = [1.0, 2.0, 3.0, 20.0]
    # 17 s between events 2 and 3 at 6e-3: a reach of 1225 -- refused without wide=, and with it beside a step cost
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, max_rate=6e-3)
    assert "event 3" in str(e.value) and "1225" in str(e.value) and "1024" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, max_rate=6e-3, step_cost=1e-4, wide=True)
    assert "event 3" in str(e.value) and "1225" in str(e.value) and "0.0001" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, max_rate=0.2, wide=True)
    assert "event 3" in str(e.value) and "40801" in str(e.value) and "32767" in str(e.value)
    need = track.TrackState.nbytes(4, 24001, wide=True)
    with pytest.raises(SushiError) as e:
        track.find_track(stream, patterns, centres, 1.0, 0.5, max_rate=6e-3, wide=True, max_state_bytes=need - 1)
    assert str(need) in str(e.value) and "window records" in str(e.value)
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


def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    names = {"sushi_hip_track_wide_bytes", "sushi_hip_track_margins_wide_bytes", "sushi_hip_track_forward_wide",
             "sushi_hip_track_forward_wide_keep", "sushi_hip_track_margins_wide"}
    assert names <= set(_native.declared_symbols()) and L.sushi_hip_abi_version() == 13
    pad = lambda b: (b + 255) // 256 * 256
    for n in (1, 499, 240001):
        records = 2 * pad(8 * n) + 2 * pad(4 * n)
        assert L.sushi_hip_track_wide_bytes(3, n) == L.sushi_hip_track_bytes(3, n) + records == \
            L.sushi_hip_track_bytes(3, n) + track.wide_workspace_bytes(n)
        assert L.sushi_hip_track_margins_wide_bytes(3, n) == L.sushi_hip_track_margins_bytes(3, n) + records
    for bad in ((0, 5), (5, 0), (-1, -1)):
        assert L.sushi_hip_track_wide_bytes(*bad) == 0 and L.sushi_hip_track_margins_wide_bytes(*bad) == 0
    rows = np.array([(0, 1.0), (501, 0.0), (333, 2.5)], dtype=_native.JOINT_ROW_DTYPE)
    reach = np.array([0, 32767, 1025, 2000], np.int32)
    guard = np.array([0, 120, 5], np.int32)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first
    odd = ctypes.c_void_p((1 << 20) + 128)
    EINVAL, EALIGN, ENOSPACE = -1, -2, _native.ENOSPACE

    def forward(fn, reach=reach, step_cost=0.0, row0=2, mem=P, mem_bytes=16, D=P):
        return fn(P, 1000, rows.ctypes.data, reach.ctypes.data, 3, 499, 0, 0.5, step_cost, row0, 7, D, P, P, P, P, P, mem, mem_bytes, None)

    def margins(fn, reach=reach, step_cost=0.0, row0=2, mem=P, mem_bytes=16):
        return fn(P, 1000, rows.ctypes.data, reach.ctypes.data, guard.ctypes.data, 3, 499, 0, 0.5, step_cost, row0, 7, P, P, P, P, P, P,
                  P, P, P, None, mem, mem_bytes, None)

    def changed(at, value):
        r = reach.copy()
        r[at] = value
        return r

    for call, fns in ((forward, (L.sushi_hip_track_forward_wide, L.sushi_hip_track_forward_wide_keep)),
                      (margins, (L.sushi_hip_track_margins_wide,))):
        for fn in fns:
            assert call(fn) == ENOSPACE                                   # good arguments: the workspace is what fails
            assert call(fn, step_cost=-0.0) == ENOSPACE
            assert call(fn, reach=changed(1, 32768)) == EINVAL            # reach_32768, before the workspace ...
            assert call(fn, reach=changed(1, 32768), mem=odd) == EINVAL   # ... and before its alignment
            assert call(fn, reach=changed(2, -1)) == EINVAL
            assert call(fn, step_cost=1e-3) == EINVAL                     # wide_reach_with_step_cost
            assert call(fn, step_cost=1e-3, mem=odd) == EINVAL
            assert call(fn, reach=np.array([0, 1024, 7, 1024], np.int32), step_cost=1e-3) == ENOSPACE
            assert call(fn, mem=odd) == EALIGN
            assert call(fn, mem_bytes=L.sushi_hip_track_bytes(3, 499)) == ENOSPACE       # the plain call's workspace is too small
    # reach[0]: used by a forward call that continues a sequence, ignored in the sequence's row 0, never used by a margins call
    assert forward(L.sushi_hip_track_forward_wide, reach=changed(0, 32768)) == EINVAL
    assert forward(L.sushi_hip_track_forward_wide, reach=changed(0, 32768), row0=0) == ENOSPACE
    assert margins(L.sushi_hip_track_margins_wide, reach=changed(0, 32768)) == ENOSPACE
    # reach[3]: the row after a margins call that ends below the sequence's last row
    assert margins(L.sushi_hip_track_margins_wide, reach=changed(3, 32768)) == EINVAL
    assert margins(L.sushi_hip_track_margins_wide, reach=changed(3, 32768), row0=4) == ENOSPACE
    assert forward(L.sushi_hip_track_forward_wide, D=ctypes.c_void_p((1 << 20) + 4), mem_bytes=1 << 30) == EALIGN
    # the plain entry points keep their bound
    assert forward(L.sushi_hip_track_forward, reach=changed(1, 1025)) == EINVAL
    assert forward(L.sushi_hip_track_forward_keep, reach=changed(1, 1025)) == EINVAL
    assert margins(L.sushi_hip_track_margins, reach=changed(1, 1025)) == EINVAL
    assert forward(L.sushi_hip_track_forward, reach=np.array([0, 1024, 7, 0], np.int32)) == ENOSPACE


# ---------------------------------------------------------------------------------------------- the kernels' header on the CPU
EXPECTED_RC = {   # case of host_track_wide_check validate -> what stage_track_wide and stage_margins_wide return
    "good": (0, 0), "step_cost_neg_zero": (0, 0), "narrow_reaches_with_step_cost": (0, 0), "reach_32768": (-1, -1),
    "reach_negative": (-1, -1), "reach_int_max": (-1, -1), "wide_reach_with_step_cost": (-1, -1),
    "reach_1025_with_step_cost": (-1, -1), "first_reach_32768": (-1, 0), "first_reach_wide_with_step_cost": (-1, 0),
    "reach_of_row_0_is_ignored": (0, 0), "reach_after_the_call_32768": (0, -1), "reach_after_the_sequence_is_ignored": (0, 0),
    "reach_after_the_call_wide_with_step_cost": (0, -1), "guard_negative": (0, -1), "penalty_nan": (-1, -1),
    "step_cost_negative": (-1, -1), "row_one_past_curves_end": (-1, -1), "reach_32768_before_workspace": (-1, -1),
    "wide_reach_with_step_cost_before_alignment": (-1, -1), "workspace_misaligned_and_short": (-2, -2),
    "workspace_exact_forward": (0, 0), "workspace_exact_margins": (0, 0), "workspace_short": (-4, -4),
    "workspace_of_the_plain_call": (-4, -4)}


def test_stage_wide_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = {l.split()[0]: (int(l.split()[1]), int(l.split()[2])) for l in lines[:len(EXPECTED_RC)]}
    assert got == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    pad = lambda b: (b + 255) // 256 * 256
    records = lambda n: 2 * pad(8 * n) + 2 * pad(4 * n)
    assert rest[0] == "bytes %d %d %d 0 0 0" % (512 + records(1), 18944 + records(240001), 2 * 28160 + records(2880001))
    assert rest[1] == "margin_bytes %d %d 0 0" % (512 + records(1), 2 * pad(36 * 469) + records(240001))
    # a window tile is 1024 values, four to a thread; a work item asks for at most 67 whole tiles' records (66 are met)
    assert rest[2] == "tile 1024 per=4 item_tiles=67 tiles=1,1,2 grid=235,2048"
    assert rest[3] == ("facts_240001 rc=0 per=2 items=469 grid=469 plain=18944 records=(18944,%d,%d,%d) bytes=%d tile_grid=235 wide_rows=1"
                       % (18944 + pad(8 * 240001), 18944 + 2 * pad(8 * 240001), 18944 + 2 * pad(8 * 240001) + pad(4 * 240001),
                          18944 + records(240001)))
    assert rest[4] == "most_item_tiles 66" and len(rest) == 5


def _near_by_check(check, tmp_path, D, reach, mu, mode="near"):
    paths = [os.path.join(str(tmp_path), name) for name in ("row", "out")]
    np.ascontiguousarray(D, np.float64).tofile(paths[0])
    subprocess.check_call([check, mode, float(mu).hex(), str(reach), paths[0], paths[1]])       # (exit status 4: it met a difference)
    raw = np.fromfile(paths[1], np.uint8)
    n = D.shape[0]
    return raw[:8 * n].view(np.float64), raw[8 * n:].view(np.int16)


def test_the_header_on_the_cpu_equals_the_candidate_loop(check, tmp_path):
    """wide_combine, the tile pass as the kernel divides it, the staged tile records and wide_near over whole rows, inside the
    program against track_core.hpp's candidate loop and here against _near_wide: the sizes around one, two and four window tiles,
    a reach wider than the axis, the widest reach, every kind of tie."""
    for n, reach in ((1, 1025), (2, 32767), (1025, 1025), (1026, 1025), (2053, 2048), (3079, 1500), (4104, 2049), (5000, 4999),
                     (5000, 32767)):
        for k, kind in enumerate(cases.KINDS):
            D = cases.tie_row(n, kind, seed=4) * (1.0, -1.0)[k % 2]
            mu = (0.0, -0.0)[(k // 2) % 2]
            near, words = _near_by_check(check, tmp_path, D, reach, mu)
            want, want_d = track._near_wide(D, reach, mu, moves=True)
            assert (_bits64(near) == _bits64(want)).all() and (words == want_d).all(), (n, reach, kind)
    # an axis longer than twice the widest reach: the work items in the middle stage 66 whole tiles' records, from both sides.  The
    # program's own candidate loop over 70001 x 65534 candidates takes too long under the sanitizers: `near_only` leaves it out, and
    # the comparison is the one here, with _near_wide (which the tests above hold against the loop)
    for kind, mu in (("few_values", 0.0), ("zeros", -0.0), ("random", 0.0)):
        D = cases.tie_row(70001, kind, seed=1)
        near, words = _near_by_check(check, tmp_path, D, 32767, mu, mode="near_only")
        want, want_d = track._near_wide(D, 32767, mu, moves=True)
        assert (_bits64(near) == _bits64(want)).all() and (words == want_d).all(), kind


@pytest.mark.parametrize("method", METHODS)
def test_the_header_on_the_cpu_equals_track_host(check, tmp_path, method):
    E, n = 5, 4104
    curves, rows, weights = cases.sequence(E, n, method, seed=9)
    rt = np.array(rows, dtype=_native.JOINT_ROW_DTYPE)
    paths = [os.path.join(str(tmp_path), name) for name in ("curves", "rows", "reach", "out")]
    curves.tofile(paths[0])
    rt.tofile(paths[1])
    np.array(cases.MIXED_REACH, np.int32).tofile(paths[2])
    subprocess.check_call([check, "pass", method.split("_")[0], float(0.0625).hex(), float(-0.0).hex(), str(n)] + paths)
    raw = np.fromfile(paths[3], np.uint8)
    want = track.track_host(cases.rows_of(curves, rows, n), weights, 0.0625, -0.0, cases.MIXED_REACH, method, wide=True)
    assert raw[:4 * E].view(np.int32).tolist() == want.shifts.tolist() and raw[4 * E:8 * E].view(np.int32).tolist() == want.row_arg.tolist()
    assert (raw[8 * E:16 * E].view(np.uint64) == _bits64(want.row_min)).all()
    assert (raw[16 * E:].view(np.int16).reshape(E, n) == want.moves).all()


# ---------------------------------------------------------------------------------------------- the long-gap scenario on the oracle
@pytest.fixture(scope="module")
def gap_case(oracle):
    """The CPU oracle's rows of the long-gap scenario (tests/track_wide_cases.py), without and with event 5's decoy."""
    import segment_cases
    from sushi_amd import joint
    out = {}
    for decoy in (False, True):
        dst, src = cases.gap_streams(decoy)
        patterns, _centres, bases = cases.gap_scenario(dst, src)
        window = joint.joint_window(bases, [p.shape[1] for p in patterns], dst.data.shape[1], int(cases.GAP_RATE * cases.GAP_WINDOW))
        assert window == (cases.GAP_K_LO, cases.GAP_N_SHIFT)
        assert track.rate_reach(bases, cases.GAP_MAX_RATE, cases.GAP_SLACK) == cases.GAP_REACH
        out[decoy] = segment_cases.oracle_rows(oracle, dst, patterns, bases, cases.GAP_K_LO, cases.GAP_N_SHIFT)
    return out


def _shifts_and_jumps(got):
    return (got.shifts + cases.GAP_K_LO).tolist(), [e for e in range(1, 10) if got.moves[e, got.shifts[e]] == JUMP]


def test_the_wide_pass_walks_a_long_gap_that_a_clipped_reach_jumps(oracle, gap_case):
    """Ten events, 21.3 s without one in front of event 5, a drift of 1890 samples across it; max_rate 9e-3 gives reach_5 = 2399.
    Penalties tried: 0.02, 0.05, 0.1, 0.25, 0.5, 1.0, 2.0 (tests/track_wide_cases.py says what holds where).
    * wide=False refuses the reach, naming the event;
    * clipped to 1024 the pass cannot walk 1890 samples: without a decoy it still finds the ten true shifts -- at every penalty
      tried, which is said here and not hidden -- but enters event 5 by a jump, and its cost is the wide pass's plus the penalty;
    * with event 5's decoy planted 610 samples from event 4's shift, the clipped pass walks to the decoy for nothing and pays its
      jump one event later: wrong at all seven penalties;
    * wide=True returns the ten true shifts and no jump at all -- without the decoy at all seven penalties, with it from 0.25 on (below
      that the noise at the true place, 0.164 of score, costs more than a jump back: no reach changes that, and it is asserted too)."""
    plain, decoyed = gap_case[False], gap_case[True]
    assert cases.GAP_REACH[5] == 2399 and cases.GAP_CLIPPED[5] == 1024 and abs(cases.GAP_TRUE_K[5] - cases.GAP_TRUE_K[4]) == 1890
    assert [oracle.argmin_first(r) + cases.GAP_K_LO for r in plain] == cases.GAP_TRUE_K
    assert [oracle.argmin_first(r) + cases.GAP_K_LO for r in decoyed] == cases.GAP_DECOY_K          # a lone search prefers the clean copy
    w = [1.0] * 10
    for rows in (plain, decoyed):
        with pytest.raises(SushiError) as e:
            track.track_host(rows, w, 0.5, 0.0, cases.GAP_REACH)
        assert "event 5" in str(e.value) and "2399" in str(e.value) and "1024" in str(e.value)
    for lam in cases.GAP_PENALTIES_BELOW_THE_NOISE + cases.GAP_PENALTIES:
        clipped = track.track_host(plain, w, lam, 0.0, cases.GAP_CLIPPED)
        wide = track.track_host(plain, w, lam, 0.0, cases.GAP_REACH, wide=True)
        assert _shifts_and_jumps(clipped) == (cases.GAP_TRUE_K, [5]), lam
        assert _shifts_and_jumps(wide) == (cases.GAP_TRUE_K, []), lam
        assert wide.moves[5, wide.shifts[5]] == cases.GAP_TRUE_K[4] - cases.GAP_TRUE_K[5] == 1890
        assert abs(clipped.cost - (wide.cost + lam)) < 1e-12
        clipped = track.track_host(decoyed, w, lam, 0.0, cases.GAP_CLIPPED)
        assert _shifts_and_jumps(clipped) == (cases.GAP_DECOY_K, [6]), lam                          # on the decoy, at every penalty
        wide = track.track_host(decoyed, w, lam, 0.0, cases.GAP_REACH, wide=True)
        if lam in cases.GAP_PENALTIES:
            assert _shifts_and_jumps(wide) == (cases.GAP_TRUE_K, []), lam
            assert wide.cost < clipped.cost
        else:
            assert _shifts_and_jumps(wide) == (cases.GAP_DECOY_K, [6]), lam
    noise = float(decoyed[5][cases.GAP_TRUE_K[5] - cases.GAP_K_LO]) - float(decoyed[5][cases.GAP_DECOY_K[5] - cases.GAP_K_LO])
    assert max(cases.GAP_PENALTIES_BELOW_THE_NOISE) < noise < min(cases.GAP_PENALTIES) and abs(noise - 0.164) < 0.001
    # the margins say the same: with the decoy, at penalty 0.5, event 5's best alternative is the decoy
    m = track.track_margins_host(decoyed, w, 0.5, 0.0, cases.GAP_REACH, 120, wide=True)
    assert m.alt_arg[5] + cases.GAP_K_LO == cases.GAP_DECOY_K[5] and m.alt[5] - m.through[5] > 0.3
