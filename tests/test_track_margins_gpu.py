"""Margins on the GPU: sushi_hip_track_forward_keep against sushi_hip_track_forward and sushi_hip_track_margins against its NumPy
restatement (sushi_amd/track.py track_margins_host), bit for bit down to every min-marginal, on the synthetic sequences of
tests/track_cases.py; backward chunking; every halo variant; ties and work-item boundaries; WavStream.find_track(margins=True) on the
wandering-shift scenario against the margins recorded in tests/track_margin_cases.py; shifts.calculate_tracked_shifts; refusals."""
import numpy as np
import pytest

import track_cases as cases
import track_margin_cases as mcases
from sushi_amd import track
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, calculate_tracked_shifts

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _forward(curves_dev, rows, reach, n, lam, mu, method, keep):
    state = track.TrackState(len(rows), n, curves_dev.device, keep=keep)
    (track.track_forward_keep_device if keep else track.track_device)(curves_dev, rows, reach, lam, mu, state, method=method)
    return state, track.track_backtrack_device(state)


def _margins(curves_dev, state, shifts, rows, reach, guard, lam, mu, method, chunks=None, with_M=True):
    """The margins pass on the device: calls over `chunks` (row counts, from the sequence's last rows down; default: one call)."""
    import torch
    E, n = len(rows), state.n_shift
    M = torch.full((E * n,), float("nan"), dtype=torch.float64, device=curves_dev.device) if with_M else None
    last = E
    for count in chunks or [E]:
        first = last - count
        track.track_margins_device(curves_dev, rows[first:last], reach[first:last + 1 if last < E else last], guard[first:last], lam, mu,
                                   state, shifts, row0=first, method=method, marginals=M)
        last = first
    assert last == 0
    return M


def _run(curves, rows, reach, guard, n, lam, mu, method, chunks=None, with_M=True):
    import torch
    dev = torch.from_numpy(curves).cuda()
    state, shifts = _forward(dev, rows, reach, n, lam, mu, method, keep=True)
    return state, shifts, _margins(dev, state, shifts, rows, reach, guard, lam, mu, method, chunks, with_M)


def _assert_equals_host(state, shifts, M, want):
    E, n = want.marginals.shape
    assert shifts.cpu().numpy().tolist() == want.shifts.tolist()
    assert (_bits64(state.D.cpu().numpy().reshape(E, n)) == _bits64(want.D)).all()
    for name in ("through", "best", "alt", "c_min"):
        assert (_bits64(getattr(state, name).cpu().numpy()) == _bits64(getattr(want, name))).all(), name
    assert state.best_arg.cpu().numpy().tolist() == want.best_arg.tolist()
    assert state.alt_arg.cpu().numpy().tolist() == want.alt_arg.tolist()
    if M is not None:
        assert (_bits64(M.cpu().numpy().reshape(E, n)) == _bits64(want.marginals)).all()


def _host(curves, rows, weights, lam, mu, rs, guard, n, method):
    return track.track_margins_host(cases.rows_of(curves, rows, n), weights, lam, mu, rs, guard, method)


# ---------------------------------------------------------------------------------------------- the pass, synthetic rows
@pytest.fixture(scope="module", params=METHODS)
def sequences(request):
    """One sequence per shape of cases.SHAPES, with track_margins_host's answer: computed once."""
    out = {}
    for E, n, reach in cases.SHAPES:
        curves, rows, weights, lam, rs, mu = cases.sequence(E, n, reach, request.param, seed=3)
        guard = mcases.guards(E, n)
        out[(E, n, reach)] = (curves, rows, rs, guard, lam, mu, _host(curves, rows, weights, lam, mu, rs, guard, n, request.param))
    return request.param, out


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_forward_keep_equals_forward(sequences, shape):
    """Moves, row_min, row_arg and the own outputs are bitwise track_device's; every kept row of D is the host's."""
    import torch
    method, table = sequences
    curves, rows, rs, _guard, lam, mu, want = table[shape]
    dev = torch.from_numpy(curves).cuda()
    kept, shifts_kept = _forward(dev, rows, rs, shape[1], lam, mu, method, keep=True)
    plain, shifts_plain = _forward(dev, rows, rs, shape[1], lam, mu, method, keep=False)
    assert torch.equal(shifts_kept, shifts_plain) and shifts_kept.cpu().numpy().tolist() == want.shifts.tolist()
    for a, b in zip(kept.tensors()[1:], plain.tensors()[1:]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(kept.last_D().view(torch.int64), plain.last_D().view(torch.int64))
    assert (_bits64(kept.D.cpu().numpy().reshape(want.D.shape)) == _bits64(want.D)).all()
    assert (kept.moves.cpu().numpy().reshape(want.moves.shape) == want.moves).all()
    with pytest.raises(SushiError):
        track.track_device(dev, rows, rs, lam, mu, kept, method=method)
    with pytest.raises(SushiError):
        track.track_forward_keep_device(dev, rows, rs, lam, mu, plain, method=method)
    with pytest.raises(SushiError):
        track.track_margins_device(dev, rows, rs, 0, lam, mu, plain, shifts_plain, method=method)


def test_forward_keep_in_chunks_has_the_bits_of_one_call(sequences):
    import torch
    method, table = sequences
    curves, rows, rs, _guard, lam, mu, want = table[(33, 1023, 127)]
    dev = torch.from_numpy(curves).cuda()
    for chunks in ([1, 15, 17], [2, 31]):
        state = track.TrackState(33, 1023, dev.device, keep=True)
        row0 = 0
        for count in chunks:
            track.track_forward_keep_device(dev, rows[row0:row0 + count], rs[row0:row0 + count], lam, mu, state, row0=row0, method=method)
            row0 += count
        assert (_bits64(state.D.cpu().numpy().reshape(want.D.shape)) == _bits64(want.D)).all()
        assert (state.moves.cpu().numpy().reshape(want.moves.shape) == want.moves).all()


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_margins_equal_track_margins_host(sequences, shape):
    """(rows, shifts, reach) of cases.SHAPES: wave, workgroup and work-item edges, every halo size, a reach wider than a work item
    and wider than the axis, weights 1, 1/3, 0 and 2.5, planted ties; the guard is 0, 1, 300 and n_shift by turns.  The five
    outputs, c_min and every row of M: bitwise."""
    method, table = sequences
    curves, rows, rs, guard, lam, mu, want = table[shape]
    assert len(set(guard)) == min(4, shape[0]) and (want.alt_arg[3::4] == -1).all()
    state, shifts, M = _run(curves, rows, rs, guard, shape[1], lam, mu, method)
    _assert_equals_host(state, shifts, M, want)
    if shape[0] == 7:       # without M_dev: the same outputs
        _assert_equals_host(*_run(curves, rows, rs, guard, shape[1], lam, mu, method, with_M=False), want)


@pytest.mark.parametrize("shape", [(33, 1023, 127), (7, 64, 3)])
def test_a_sequence_in_backward_chunks_has_the_bits_of_one_call(sequences, shape):
    method, table = sequences
    curves, rows, rs, guard, lam, mu, want = table[shape]
    E = shape[0]
    for chunks in ([1] * E, [2] * (E // 2) + [E % 2] * (E % 2), [3] * (E // 3) + [E % 3] * (E % 3 > 0), [5] * (E // 5) + [E % 5] * (E % 5 > 0),
                   [E - 4, 1, 3]):      # boundaries odd and even
        assert sum(chunks) == E
        _assert_equals_host(*_run(curves, rows, rs, guard, shape[1], lam, mu, method, chunks=chunks), want)
    import torch
    dev = torch.from_numpy(curves).cuda()
    state, shifts = _forward(dev, rows, rs, shape[1], lam, mu, method, keep=True)
    with pytest.raises(SushiError):     # a call that ends before the last row carries the reach of the row after it
        track.track_margins_device(dev, rows[:2], rs[:2], guard[:2], lam, mu, state, shifts, method=method)
    with pytest.raises(SushiError):
        track.track_margins_device(dev, rows[E - 2:], rs[E - 2:], [0, -1], lam, mu, state, shifts, row0=E - 2, method=method)
    with pytest.raises(SushiError):
        track.track_margins_device(dev, rows[E - 2:], rs[E - 2:], 0, lam, mu, state, shifts, row0=E - 1, method=method)
    with pytest.raises(SushiError):
        track.track_margins_device(dev, rows, rs, 0, lam, mu, state, shifts.long(), method=method)


@pytest.mark.parametrize("method", METHODS)
def test_halo_variants_and_small_axes(method):
    """Reach 256 | 257 (two and eight rounds of halo) and 1024 on 4097 shifts; a reach above n_shift (5 and 7 shifts); E = 1;
    n_shift = 1."""
    for E, n, reach in ((3, 4097, 256), (3, 4097, 257), (3, 4097, 1024)):
        curves, rows, weights, lam, _rs, mu = cases.sequence(E, n, reach, method, seed=7)
        rs, guard = [0, reach, reach], [0, 1, 300]
        _assert_equals_host(*_run(curves, rows, rs, guard, n, lam, mu, method), _host(curves, rows, weights, lam, mu, rs, guard, n, method))
    for E, n, reach in ((3, 5, 1024), (4, 7, 64), (1, 1023, 0), (1, 1, 0), (5, 1, 3)):
        curves, rows, weights, lam, rs, mu = cases.sequence(E, n, reach, method, seed=5)
        guard = mcases.guards(E, n)[::-1]
        _assert_equals_host(*_run(curves, rows, rs, guard, n, lam, mu, method), _host(curves, rows, weights, lam, mu, rs, guard, n, method))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("centre", [511, 512])
def test_ties_and_a_guard_window_across_a_work_item_boundary(centre, method):
    """1024 shifts are two work items of 512.  tie_rows' planted ties in the window minimum; then s_e = centre with guard 1: the
    window straddles the boundary (511 | 512), and the equal values on both sides of it take the first index."""
    a, b = cases.tie_rows(1024, centre, method)
    curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b])
    rows = [(1, 1.0), (1027, 1.0)]
    for guard in ([1, 1], [0, 600]):
        want = track.track_margins_host([a, b], [1.0, 1.0], 0.5, 0.0, [0, 3], guard, method)
        _assert_equals_host(*_run(curves, rows, [0, 3], guard, 1024, 0.5, 0.0, method), want)
    # one row, E = 1: M is u.  The best value at `centre`, the second best twice, two shifts to either side of it
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    row = np.full(1024, 0.75, np.float32)
    row[centre], row[centre - 2], row[centre + 2] = 0.125, 0.25, 0.25
    want = track.track_margins_host([row * sign], [1.0], 0.5, 0.0, 0, 1, method)
    assert want.shifts.tolist() == [centre] and want.alt_arg.tolist() == [centre - 2]
    _assert_equals_host(*_run(np.concatenate([np.zeros(1, np.float32), row * sign]), [(1, 1.0)], [0], [1], 1024, 0.5, 0.0, method), want)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [cases.PER_LARGE_FROM, cases.PER_LARGE_FROM - 1])
def test_margins_at_the_size_where_the_split_changes(n, method):
    """The shifts from which on a workgroup takes eight indices per thread, and one shift below it: two rows, reach 2; the minimum
    lies twice in the last, cut item's last elements.  Without M_dev; the outputs and the C halves against the host."""
    E = 2
    rng = np.random.default_rng(19)
    lo = 0.25 if method == "sqdiff_normed" else -0.5
    curves = rng.random(E * (n + 3) + 8, dtype=np.float32) * np.float32(0.5) + np.float32(lo)
    rows = [(1 + e * (n + 3) + 2 * (e % 2), (1.0, 1.0 / 3.0)[e]) for e in range(E)]
    best = np.float32(0.125 if method == "sqdiff_normed" else 0.875)
    for o, _w in rows:
        curves[o + n - 2] = curves[o + n - 1] = best
    want = track.track_margins_host(cases.rows_of(curves, rows, n), [w for _o, w in rows], 1.0, cases.STEP_COST, [0, 2], [0, 1], method)
    assert want.shifts.tolist() == [n - 2] * E and want.alt_arg.tolist() == [n - 1, n - 4]
    _assert_equals_host(*_run(curves, rows, [0, 2], [0, 1], n, 1.0, cases.STEP_COST, method, with_M=False), want)


# ---------------------------------------------------------------------------------------------- find_track
@pytest.fixture(scope="module")
def wander():
    dst, src = cases.streams()
    patterns, centres, _bases = cases.scenario(dst, src)
    kw = dict(reach=cases.REACH, step_cost=mcases.STEP_COST)
    plain = dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, **kw)
    found = dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, margins=True, guard=mcases.GUARD, marginals=True, **kw)
    return dst, src, patterns, centres, plain, found


def test_find_track_with_margins_on_the_scenario(wander):
    """The recorded setting of tests/track_margin_cases.py: shifts, jumps and cost are exactly what margins=False returns; the
    margins and alternatives are the recorded ones (the oracle's rows, track_margins_host); three chunks give equal bits."""
    dst, _src, patterns, centres, plain, found = wander
    assert found.shifts == plain.shifts == cases.TRUE_K and found.jumps == plain.jumps == cases.JUMPS
    assert _bits64(found.cost) == _bits64(plain.cost) and found.cost == mcases.COST
    for name in ("deltas", "segments", "moves", "reach", "event_own_delta", "k_lo", "n_shift"):
        assert getattr(found, name) == getattr(plain, name), name
    for name in ("event_scores", "event_own_scores"):
        assert (_bits(getattr(found, name)) == _bits(getattr(plain, name))).all(), name
    assert found.guard == [mcases.GUARD] * 10
    assert found.event_through.tolist() == mcases.THROUGH and found.event_margin.tolist() == mcases.MARGINS
    assert found.event_alt_shift == mcases.ALT_K and found.event_alt_delta == [k / float(cases.RATE) for k in mcases.ALT_K]
    assert found.event_through.dtype == found.event_margin.dtype == np.float64
    for v in cases.VICTIMS:
        assert found.event_alt_shift[v] == cases.LONE_K[v]
    M = found.marginals
    assert M.is_cuda and tuple(M.shape) == (10, cases.N_SHIFT) and str(M.dtype) == "torch.float64"
    M = M.cpu().numpy()
    assert [float(M[e, k - cases.K_LO]) for e, k in enumerate(cases.TRUE_K)] == mcases.THROUGH
    assert [float(M[e, k - cases.K_LO]) for e, k in enumerate(mcases.ALT_K)] == mcases.ALT
    assert (M.argmin(axis=1) + cases.K_LO).tolist() == cases.TRUE_K
    chunked = dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, reach=cases.REACH, step_cost=mcases.STEP_COST, margins=True,
                             guard=[mcases.GUARD] * 10, marginals=True, max_bytes=4 * 3 * cases.N_SHIFT + 3)   # 3 + 3 + 3 + 1 events
    assert chunked.shifts == found.shifts and _bits64(chunked.cost) == _bits64(found.cost) and chunked.jumps == found.jumps
    assert chunked.event_alt_shift == found.event_alt_shift and chunked.guard == found.guard
    for name in ("event_through", "event_margin"):
        assert (_bits64(getattr(chunked, name)) == _bits64(getattr(found, name))).all(), name
    assert (_bits64(chunked.marginals.cpu().numpy()) == _bits64(M)).all()
    # the default guard: int(0.01 * sample_rate); and an event with no alternative
    default = dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, reach=cases.REACH, margins=True)
    assert default.guard == [120] * 10 and default.marginals is None
    assert (_bits64(default.event_margin) == _bits64(found.event_margin)).all()
    wide = dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, reach=cases.REACH, margins=True,
                          guard=[cases.N_SHIFT] + [mcases.GUARD] * 9)
    assert wide.event_margin[0] == np.inf and wide.event_alt_shift[0] is None and wide.event_alt_delta[0] is None
    assert wide.event_margin[1:].tolist() == mcases.MARGINS[1:]


def test_find_track_without_margins_has_none_in_the_new_fields(wander):
    plain = wander[4]
    for name in ("guard", "event_through", "event_margin", "event_alt_shift", "event_alt_delta", "marginals"):
        assert getattr(plain, name) is None, name


def test_calculate_tracked_shifts_passes_the_arguments_through(wander):
    dst, src, _patterns, _centres, _plain, found = wander
    events = [ScriptEvent(s, e) for s, e in cases.EVENTS]
    got = calculate_tracked_shifts(src, dst, events, cases.WINDOW, mcases.PENALTY, reach=cases.REACH, step_cost=mcases.STEP_COST,
                                   margins=True, guard=mcases.GUARD, marginals=True)
    assert got.shifts == found.shifts and got.guard == found.guard and got.event_alt_shift == found.event_alt_shift
    assert (_bits64(got.event_margin) == _bits64(found.event_margin)).all()
    assert (_bits64(got.marginals.cpu().numpy()) == _bits64(found.marginals.cpu().numpy())).all()
    for e, k in zip(events, cases.TRUE_K):
        assert e.shift == k / float(cases.RATE)
    off = calculate_tracked_shifts(src, dst, events, cases.WINDOW, mcases.PENALTY, reach=cases.REACH)
    assert off.event_margin is None and off.marginals is None and off.shifts == found.shifts


def test_refusals(wander):
    dst, _src, patterns, centres, _plain, _found = wander
    E, n = 10, cases.N_SHIFT
    kept = track.TrackState.nbytes(E, n, keep=True)
    assert kept == E * n * 2 + E * n * 8 + 2 * n * 8 and track.TrackState.nbytes(E, n, keep=True, marginals=True) == kept + E * n * 8
    for need, kw in ((kept, dict()), (kept + E * n * 8, dict(marginals=True))):
        with pytest.raises(SushiError) as e:
            dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, reach=cases.REACH, margins=True, max_state_bytes=need - 1, **kw)
        assert str(need) in str(e.value) and str(need - 1) in str(e.value) and "10 events" in str(e.value) and str(n) in str(e.value)
    # what fits without margins still runs without them
    assert dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, reach=cases.REACH, max_state_bytes=kept - 1).shifts == cases.TRUE_K
    for bad in ([120] * 9, [120] * 11, -1, [120] * 9 + [-1], "wide"):
        with pytest.raises(SushiError):
            dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, reach=cases.REACH, margins=True, guard=bad)
    with pytest.raises(SushiError):
        dst.find_track(patterns, centres, cases.WINDOW, mcases.PENALTY, reach=cases.REACH, guard=120)
