"""Ordered margins on the GPU: sushi_hip_track_forward_ordered_keep against sushi_hip_track_forward_ordered and the host, and
sushi_hip_track_order_margins against its NumPy restatement (sushi_amd/track.py track_ordered_margins_host), bit for bit down to every
M, the two halves of C and S, on synthetic sequences with backs, penalties and guards that vary by row; backward chunks; every
halo variant; small axes and the size where the work split changes; equal minima on both sides of a wave's, a round's and a work
item's boundary; the plain device margins where no back binds; WavStream.find_ordered_track on the decoy scenario against the host
path and the recorded values, in one chunk, in three, and with clamp=; shifts.calculate_ordered_shifts; the entry points'
refusals."""
import numpy as np
import pytest

import track_cases
import track_order_cases as ocases
import track_order_margin_cases as cases
from sushi_amd import track
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, calculate_ordered_shifts

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP, ANY = -32768, -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _forward(curves_dev, rows, reach, lams, back, n, mu, method, chunks=None):
    """The ordered forward pass with its rows kept, over `chunks` (row counts; default: one call), then the backtrack."""
    state = track.TrackState(len(rows), n, curves_dev.device, ordered=True, margins=True)
    row0 = 0
    for count in chunks or [len(rows)]:
        track.track_ordered_keep_device(curves_dev, rows[row0:row0 + count], reach[row0:row0 + count], lams[row0:row0 + count], mu,
                                        back[row0:row0 + count], state, row0=row0, method=method)
        row0 += count
    assert row0 == len(rows)
    return state, track.track_ordered_backtrack_device(state)


def _margins(curves_dev, rows, reach, lams, back, guard, mu, method, state, shifts, chunks=None, marginals=True):
    """The backward walk over `chunks` (row counts from the last row down; default: one call) -> M as [E, n] (or None)."""
    import torch
    E, n = len(rows), state.n_shift
    M = torch.full((E * n,), float("nan"), dtype=torch.float64, device=curves_dev.device) if marginals else None
    last = E
    for count in chunks or [E]:
        first = last - count
        upto = last + 1 if last < E else last
        track.track_ordered_margins_device(curves_dev, rows[first:last], reach[first:upto], guard[first:last], lams[first:upto], mu,
                                           back[first:upto], state, shifts, row0=first, method=method, marginals=M)
        last = first
    assert last == 0
    return None if M is None else M.view(E, n)


def _host(curves, rows, weights, lams, mu, rs, back, guard, n, method):
    trace = []
    want = track.track_ordered_margins_host(track_cases.rows_of(curves, rows, n), weights, lams, mu, rs, back, guard, method, _trace=trace)
    return want, {e: (c, s) for e, c, s in trace}


def _assert_forward_equals_host(state, shifts, want):
    assert shifts.cpu().numpy().tolist() == want.shifts.tolist()
    row_min = state.row_min.cpu().numpy()
    assert (_bits64(row_min) == _bits64(want.row_min)).all() and _bits64(row_min[-1]) == _bits64(want.cost)
    assert state.row_arg.cpu().numpy().tolist() == want.row_arg.tolist()
    assert state.row_own_index.cpu().numpy().tolist() == want.row_own_index.tolist()
    assert (_bits(state.row_own_scores.cpu().numpy()) == _bits(want.row_own_scores)).all()
    assert (state.moves.cpu().numpy().reshape(want.moves.shape) == want.moves).all()
    assert (state.prefix_arg.cpu().numpy().reshape(want.prefix_arg.shape) == want.prefix_arg).all()
    assert (_bits64(state.D.cpu().numpy().reshape(want.D.shape)) == _bits64(want.D)).all()          # every row of D
    assert (_bits64(state.last_D().cpu().numpy()) == _bits64(want.D[-1])).all()
    assert (_bits64(state.P.cpu().numpy()) == _bits64(want.D[-1][want.prefix_arg[-1]])).all()


def _assert_margins_equal_host(state, M, want, by_row):
    E, n = want.marginals.shape
    for name in ("c_min", "through", "best", "alt"):
        assert (_bits64(getattr(state, name).cpu().numpy()) == _bits64(getattr(want, name))).all(), name
    assert state.best_arg.cpu().numpy().tolist() == want.best_arg.tolist()
    assert state.alt_arg.cpu().numpy().tolist() == want.alt_arg.tolist()
    if M is not None:
        assert (_bits64(M.cpu().numpy()) == _bits64(want.marginals)).all()
    C = state.C.cpu().numpy().reshape(2, n)
    assert (_bits64(C[0]) == _bits64(by_row[0][0])).all() and (_bits64(state.S.cpu().numpy()) == _bits64(by_row[0][1])).all()
    if E > 1:
        assert (_bits64(C[1]) == _bits64(by_row[1][0])).all()


def _whole(curves, rows, weights, lams, mu, rs, back, guard, n, method, chunks=None, marginals=True):
    """Forward, backtrack and margins on the device against the host: everything, bitwise."""
    import torch
    want, by_row = _host(curves, rows, weights, lams, mu, rs, back, guard, n, method)
    dev = torch.from_numpy(curves).cuda()
    state, shifts = _forward(dev, rows, rs, lams, back, n, mu, method)
    _assert_forward_equals_host(state, shifts, want)
    M = _margins(dev, rows, rs, lams, back, guard, mu, method, state, shifts, chunks=chunks, marginals=marginals)
    _assert_margins_equal_host(state, M, want, by_row)
    return want


# ---------------------------------------------------------------------------------------------- the passes, synthetic rows
@pytest.fixture(scope="module", params=METHODS)
def sequences(request):
    """One sequence per shape of track_cases.SHAPES, with track_ordered_margins_host's answer: computed once."""
    out = {}
    for E, n, reach in track_cases.SHAPES:
        curves, rows, weights, lams, rs, mu, back, guard = cases.sequence(E, n, reach, request.param, seed=3)
        out[(E, n, reach)] = (curves, rows, rs, lams, mu, back, guard) + _host(curves, rows, weights, lams, mu, rs, back, guard, n,
                                                                                 request.param)
    return request.param, out


@pytest.mark.parametrize("shape", track_cases.SHAPES)
def test_keep_and_margins_equal_the_host(sequences, shape):
    """track_cases.SHAPES -- wave, workgroup and work-item edges, every halo size (reach 0, <= 256, <= 1024, and a reach above
    n_shift), E = 1, rows at odd offsets, weights 1, 1/3, 0 and 2.5 -- with track_order_cases' backs and penalties and guards 0, 1, 300
    and n by turns.  forward_ordered_keep: every output of forward_ordered's, and every row of D; margins: every M, both halves of C,
    S, and the six per-row outputs: bitwise.  forward_ordered_keep also equals forward_ordered on the device."""
    import torch
    method, table = sequences
    curves, rows, rs, lams, mu, back, guard, want, by_row = table[shape]
    E, n = shape[0], shape[1]
    dev = torch.from_numpy(curves).cuda()
    state, shifts = _forward(dev, rows, rs, lams, back, n, mu, method)
    _assert_forward_equals_host(state, shifts, want)
    plain = track.TrackState(E, n, dev.device, ordered=True)
    track.track_ordered_device(dev, rows, rs, lams, mu, back, plain, method=method)
    assert torch.equal(shifts, track.track_ordered_backtrack_device(plain))
    for a, b in zip(state.tensors()[1:] + state.order_tensors()[:2], plain.tensors()[1:] + plain.order_tensors()[:2]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(state.last_D().view(torch.int64), plain.last_D().view(torch.int64))
    M = _margins(dev, rows, rs, lams, back, guard, mu, method, state, shifts)
    _assert_margins_equal_host(state, M, want, by_row)
    # without M_dev: the same outputs
    again, shifts2 = _forward(dev, rows, rs, lams, back, n, mu, method)
    assert _margins(dev, rows, rs, lams, back, guard, mu, method, again, shifts2, marginals=False) is None
    _assert_margins_equal_host(again, None, want, by_row)


@pytest.mark.parametrize("shape", [(33, 1023, 127), (7, 64, 3)])
def test_chunks_have_the_bits_of_one_call(sequences, shape):
    """The forward pass cut into chunks, and backward chunks of 1, 2, 3 and 5 rows (both parities of the boundary)."""
    import torch
    method, table = sequences
    curves, rows, rs, lams, mu, back, guard, want, by_row = table[shape]
    E, n = shape[0], shape[1]
    dev = torch.from_numpy(curves).cuda()
    for chunks in ([1] * E, [3] * (E // 3) + ([E % 3] if E % 3 else []), [2, E - 2]):
        state, shifts = _forward(dev, rows, rs, lams, back, n, mu, method, chunks=chunks)
        _assert_forward_equals_host(state, shifts, want)
    for size in (1, 2, 3, 5):
        chunks = [size] * (E // size) + ([E % size] if E % size else [])
        M = _margins(dev, rows, rs, lams, back, guard, mu, method, state, shifts, chunks=chunks)
        _assert_margins_equal_host(state, M, want, by_row)
    M = _margins(dev, rows, rs, lams, back, guard, mu, method, state, shifts, chunks=[E - 2, 2])
    _assert_margins_equal_host(state, M, want, by_row)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_small_axes(n, method):
    """n_shift 1, 2 and around one wave's four; reach 1, 0, E = 1, and a reach above n_shift (300: the wider halo variant too)."""
    for E, reach, seed in ((5, 1, 1), (8, 0, 2), (1, 0, 3), (4, 300, 4)):
        rng = np.random.default_rng(n * 31 + seed)
        lo = 0.25 if method == "sqdiff_normed" else -0.5
        curves = rng.random(E * (n + 2) + 3, dtype=np.float32) * np.float32(0.5) + np.float32(lo)
        rows = [(1 + e * (n + 2), (1.0, 1.0 / 3.0, 0.0, 2.5)[e % 4]) for e in range(E)]
        lams, back, rs = [0.0] + ocases.penalties(E, 0.0625)[1:], ocases.backs(E, n), [0] + [reach] * (E - 1)
        _whole(curves, rows, [w for _o, w in rows], lams, track_cases.STEP_COST, rs, back, cases.guards(E, n), n, method,
               chunks=None if E < 3 else [2, E - 2])


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("at", [256, 512])
def test_equal_minima_on_both_sides_of_a_boundary(at, method):
    """C_2's minimum twice, at at - 1 | at: the two sides of a wave's and a round's boundary (256) and of a work item's (512).  S is
    the minimum up to and including `at`, above it not; with back 0 t' is j itself, with back 1 one below, with back `at` index 0
    for every j up to `at`: t' lands on each side.  A guard window across the work item's boundary."""
    a, b, c = cases.suffix_tie_rows(1024, at, method)
    curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b, np.zeros(1, np.float32), c])
    rows = [(1, 1.0), (1027, 1.0), (2052, 1.0)]
    for back in (0, 1, at, ANY):
        want = _whole(curves, rows, [1.0] * 3, [0.0, 0.0625, 0.0625], 0.0, [0, 0, 0], [ANY, back, back], [0, 5, 2000], 1024, method)
        assert want.c_min[2] == 0.25                    # (the weighted cost: negated back under 'ccoeff_normed')
    # a guard window that straddles the boundary between two work items (511 | 512), and one that ends exactly at it
    for guard in ([3, 3, 3], [at - 1, 1, 0]):
        want = _whole(curves, rows, [1.0] * 3, [0.0, 0.0625, 0.0625], 0.0, [0, 0, 0], [ANY, 1, 1], guard, 1024, method)
        assert (want.alt_arg >= 0).all()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [track_cases.PER_LARGE_FROM - 1, track_cases.PER_LARGE_FROM])
def test_at_the_size_where_the_split_changes(n, method):
    """track_cases.PER_LARGE_FROM shifts: 1024 work items of 2048, eight scan rounds each, four rounds of 256 records in the scan of
    the items; one shift fewer: 4092 items of 512 over a grid of 2048.  Three rows, reach 2, back 256; the last row rises from 0.25
    to 0.75 in steps, so that records of the suffix minimum lie all along the axis."""
    E = 3
    rng = np.random.default_rng(29)
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    curves = np.empty(E * (n + 3) + 8, np.float32)
    rows = [(1 + e * (n + 3) + 2 * (e % 2), (1.0, 1.0 / 3.0, 1.0)[e]) for e in range(E)]
    ramp = np.float32(0.25) + (np.arange(n) // 1000).astype(np.float32) * np.float32(0.5 / (n // 1000 + 1))
    curves[:] = np.float32(0.5) * sign
    for e in (0, 1):
        curves[rows[e][0]:rows[e][0] + n] = (rng.random(n, dtype=np.float32) * np.float32(0.25) + np.float32(0.5)) * sign
    curves[rows[2][0]:rows[2][0] + n] = (ramp + rng.random(n, dtype=np.float32) * np.float32(2.0 ** -12)) * sign
    lams, back = [0.0, 2.0 ** -13, 2.0 ** -13], [ANY, 256, 256]
    want = _whole(curves, rows, [w for _o, w in rows], lams, track_cases.STEP_COST, [0, 2, 2], back, [0, 300, n // 2], n, method,
                  chunks=[1, 2])
    free = track.track_ordered_margins_host(track_cases.rows_of(curves, rows, n), [w for _o, w in rows], lams, track_cases.STEP_COST,
                                            [0, 2, 2], ANY, [0, 300, n // 2], method)
    assert np.count_nonzero(free.marginals[1] < want.marginals[1]) > n // 8         # the back binds all along the axis


def test_without_a_limit_they_are_the_plain_device_margins(sequences):
    """Fact 4 on the device: every back without a limit (or >= n_shift - 1) and one penalty: every output the two calls share equals
    track_forward_keep_device + track_backtrack_device + track_margins_device bitwise."""
    import torch
    method, _table = sequences
    for E, n, reach in ((33, 1023, 127), (16, 70001, 5), (7, 64, 3), (1, 1, 0)):
        curves, rows, _weights, lam, rs, mu = track_cases.sequence(E, n, reach, method, seed=3)
        guard = cases.guards(E, n)
        dev = torch.from_numpy(curves).cuda()
        ref = track.TrackState(E, n, dev.device, keep=True)
        track.track_forward_keep_device(dev, rows, rs, lam, mu, ref, method=method)
        ref_shifts = track.track_backtrack_device(ref)
        ref_M = torch.empty(E * n, dtype=torch.float64, device=dev.device)
        track.track_margins_device(dev, rows, rs, guard, lam, mu, ref, ref_shifts, method=method, marginals=ref_M)
        for back in ([ANY] * E, [ANY] + [n - 1 + (e % 2) for e in range(1, E)]):
            got, shifts = _forward(dev, rows, rs, [lam] * E, back, n, mu, method)
            assert torch.equal(shifts, ref_shifts)
            M = _margins(dev, rows, rs, [lam] * E, back, guard, mu, method, got, shifts)
            assert torch.equal(M.reshape(-1).view(torch.int64), ref_M.view(torch.int64))
            assert torch.equal(got.D.view(torch.int64), ref.D.view(torch.int64))
            for a, b in zip(got.margin_tensors()[1:], ref.margin_tensors()[1:]):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            written = 2 * n if E > 1 else n         # (one row writes half 0 of C alone)
            assert torch.equal(got.C[:written].view(torch.int64), ref.C[:written].view(torch.int64))


def test_the_entry_points_refuse(sequences):
    import torch
    method, table = sequences
    curves, rows, rs, lams, mu, back, guard, _want, _by_row = table[(7, 64, 3)]
    dev = torch.from_numpy(curves).cuda()
    state, shifts = _forward(dev, rows, rs, lams, back, 64, mu, method)
    ordered = track.TrackState(7, 64, dev.device, ordered=True)
    kept = track.TrackState(7, 64, dev.device, keep=True)
    args = lambda **kw: dict(dict(curves=dev, rows=rows[4:], reach=rs[4:], guard=guard[4:], penalties=lams[4:], step_cost=mu,
                                  back=back[4:], state=state, shifts=shifts, row0=4, method=method), **kw)
    track.track_ordered_margins_device(**args())
    for bad in (dict(state=ordered), dict(state=kept), dict(row0=5), dict(row0=-1), dict(reach=rs[4:6]), dict(penalties=lams[4:6]),
                dict(back=back[4:6]), dict(guard=[0, 0]), dict(guard=[0, -1, 0]), dict(back=[0, -2, 0]), dict(penalties=[0.0, -1.0, 0.5]),
                dict(penalties=[0.0, float("nan"), 0.5]), dict(reach=[0, 1025, 0]), dict(shifts=shifts.cpu()), dict(shifts=shifts[:6]),
                dict(marginals=torch.empty(7 * 64, dtype=torch.float32, device=dev.device)),
                dict(marginals=torch.empty(7 * 63, dtype=torch.float64, device=dev.device)), dict(step_cost=-1.0)):
        with pytest.raises(SushiError):
            track.track_ordered_margins_device(**args(**bad))
    # a call below the last row takes one more reach, back and penalty: the step out of its last row
    with pytest.raises(SushiError) as e:
        track.track_ordered_margins_device(**args(rows=rows[2:4], guard=guard[2:4], reach=rs[2:4], penalties=lams[2:5], back=back[2:5],
                                                  row0=2))
    assert "3 are needed" in str(e.value)
    with pytest.raises(SushiError):
        track.track_ordered_keep_device(dev, rows, rs, lams, mu, back, ordered, method=method)       # a state that keeps no rows
    with pytest.raises(SushiError):
        track.track_ordered_device(dev, rows, rs, lams, mu, back, state, method=method)              # ... and one that does
    with pytest.raises(SushiError):
        track.track_ordered_keep_device(dev, rows, rs, lams, mu, back, kept, method=method)
    with pytest.raises(SushiError):
        track.track_device(dev, rows, rs, 0.5, mu, state, method=method)
    with pytest.raises(SushiError):
        track.TrackState(7, 64, dev.device, keep=True, ordered=True)


# ---------------------------------------------------------------------------------------------- find_ordered_track
@pytest.fixture(scope="module")
def decoys():
    dst, src = ocases.streams()
    patterns, centres, bases = ocases.scenario(dst, src)
    return dst, src, patterns, centres, bases


def _assert_track_margins_equal(found, want, guard, k_lo, rate):
    assert [k - k_lo for k in found.shifts] == want.shifts.tolist() and _bits64(found.cost) == _bits64(want.cost)
    assert found.guard == [guard] * len(found.shifts)
    assert (_bits64(found.event_through) == _bits64(want.through)).all()
    assert (_bits64(found.event_margin) == _bits64(np.where(want.alt_arg < 0, np.inf, want.alt - want.through))).all()
    assert found.event_alt_shift == [None if k < 0 else k_lo + int(k) for k in want.alt_arg]
    assert found.event_alt_delta == [None if k is None else k / float(rate) for k in found.event_alt_shift]
    assert found.marginals.shape == want.marginals.shape
    assert (_bits64(found.marginals.cpu().numpy()) == _bits64(want.marginals)).all()


@pytest.mark.parametrize("method", METHODS)
def test_find_ordered_track_with_margins_on_the_decoy_scenario(decoys, method):
    """tests/test_track_order_margins_host.py's scenario: find_ordered_track(margins=True, marginals=True) equals the host path over
    match_templates rows bitwise -- in one chunk and in three; under 'sqdiff_normed' also the values recorded from the oracle; under
    'ccoeff_normed' also with clamp=0.5 against the host on the clamped rows.  With margins=False it is find_track(order=True) field by
    field, and the margins' fields are None."""
    dst, _src, patterns, centres, bases = decoys
    rows = [r[0] for r in dst.match_templates(patterns, centres, [ocases.WINDOW] * 10, method=method)]
    back = track.order_back(bases, [p.shape[1] for p in patterns])
    want = track.track_ordered_margins_host(rows, [1.0] * 10, ocases.PENALTY, 0.0, 0, back, cases.GUARD, method)
    call = lambda **kw: dst.find_ordered_track(patterns, centres, ocases.WINDOW, ocases.PENALTY, order=True, reach=0, method=method, **kw)
    found = call(margins=True, marginals=True)
    assert (found.k_lo, found.n_shift) == (ocases.K_LO, ocases.N_SHIFT)
    assert found.back == ocases.BACK and found.penalties == [0.0] + [ocases.PENALTY] * 9
    _assert_track_margins_equal(found, want, cases.GUARD, ocases.K_LO, ocases.RATE)
    chunked = call(margins=True, marginals=True, max_bytes=4 * 4 * ocases.N_SHIFT + 3)
    _assert_track_margins_equal(chunked, want, cases.GUARD, ocases.K_LO, ocases.RATE)
    assert chunked.shifts == found.shifts and (_bits(chunked.event_scores) == _bits(found.event_scores)).all()
    without = call(margins=True)
    assert without.marginals is None and (_bits64(without.event_margin) == _bits64(found.event_margin)).all()
    # margins=False: find_track(order=True), field by field; the margins' fields are None
    off = call()
    ref = dst.find_track(patterns, centres, ocases.WINDOW, ocases.PENALTY, reach=0, order=True, method=method)
    assert sorted(vars(off)) == sorted(vars(ref))
    for name, a in vars(ref).items():
        b = getattr(off, name)
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), name
        else:
            assert a == b, name
    for name in ("guard", "event_through", "event_margin", "event_alt_shift", "event_alt_delta", "marginals"):
        assert getattr(off, name) is None
    for name in ("shifts", "deltas", "jumps", "segments", "cost", "back", "penalties", "reach", "moves"):
        assert getattr(found, name) == getattr(off, name), name
    if method == "sqdiff_normed":
        assert found.shifts == ocases.TRUE_K and found.cost == cases.COST
        assert found.event_through.tolist() == cases.THROUGH and found.event_margin.tolist() == cases.MARGINS
        assert found.event_alt_shift == cases.ALT_K
        listed = dst.find_ordered_track(patterns, centres, ocases.WINDOW, [ocases.PENALTY] * 10, order=ocases.BACK, reach=0, margins=True,
                                        guard=[cases.GUARD] * 10)
        assert (_bits64(listed.event_margin) == _bits64(found.event_margin)).all() and listed.event_alt_shift == found.event_alt_shift
        need = track.TrackState.nbytes(10, ocases.N_SHIFT, ordered=True, margins=True)
        with pytest.raises(SushiError) as e:
            call(margins=True, max_state_bytes=need - 1)
        assert str(need) in str(e.value)
        with pytest.raises(SushiError):
            call(guard=5)
    else:
        f = np.float32(0.5)
        clamped = [np.where(r >= f, r, f) for r in rows]
        want = track.track_ordered_margins_host(clamped, [1.0] * 10, ocases.PENALTY, 0.0, 0, back, cases.GUARD, method)
        for kw in (dict(), dict(max_bytes=4 * 4 * ocases.N_SHIFT + 3)):
            got = call(margins=True, marginals=True, clamp=0.5, **kw)
            _assert_track_margins_equal(got, want, cases.GUARD, ocases.K_LO, ocases.RATE)
            assert got.clamp == 0.5 and got.rows_info is not None
            assert (_bits(got.event_scores) == _bits([r[s] for r, s in zip(rows, want.shifts)])).all()       # the true scores


def test_calculate_ordered_shifts(decoys):
    dst, src, patterns, centres, _bases = decoys
    events = [ScriptEvent(s, e) for s, e in ocases.EVENTS]
    got = calculate_ordered_shifts(src, dst, events, ocases.WINDOW, ocases.PENALTY, reach=0, margins=True, guard=cases.GUARD)
    assert got.shifts == ocases.TRUE_K and got.jumps == [5] and got.back == ocases.BACK
    assert got.event_margin.tolist() == cases.MARGINS and got.event_alt_shift == cases.ALT_K and got.marginals is None
    assert got.guard == [cases.GUARD] * 10
    for e, k, score in zip(events, ocases.TRUE_K, got.event_scores):
        assert e.shift == k / float(ocases.RATE) and _bits(e.diff) == _bits(score) and not e.linked
    off = calculate_ordered_shifts(src, dst, events, ocases.WINDOW, ocases.PENALTY, reach=0)
    assert off.shifts == ocases.TRUE_K and off.event_margin is None and off.guard is None
    free = calculate_ordered_shifts(src, dst, events, ocases.WINDOW, ocases.PENALTY, order=None, reach=0, margins=True, marginals=True)
    assert free.shifts == ocases.RESULTS[ocases.PENALTY][0] and free.back == [None] * 10 and free.marginals.shape == (10, ocases.N_SHIFT)
    with pytest.raises(SushiError):
        calculate_ordered_shifts(src, dst, [], ocases.WINDOW, ocases.PENALTY, reach=0)
