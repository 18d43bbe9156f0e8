"""Ordered tracking on the GPU: sushi_hip_track_forward_ordered / sushi_hip_track_backtrack_ordered against their NumPy
restatement (sushi_amd/track.py track_ordered_host), bit for bit down to the moves and the jump sources, on synthetic sequences
with backs and penalties that vary by row; small axes and the size where the work split changes; chunking; today's device pass
where the backs set no limit; WavStream.find_track(order=True) on the decoy scenario of tests/test_track_order_host.py against the
host path over match_templates rows, with and without clamp=; shifts.calculate_tracked_shifts(order=True)."""
import numpy as np
import pytest

import track_cases
import track_order_cases as cases
from sushi_amd import track
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, calculate_tracked_shifts

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP, ANY = -32768, -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(curves_dev, rows, reach, lams, back, n, mu, method, chunks=None):
    """The whole pass on the device: forward calls over `chunks` (row counts; default: one call), then the backtrack."""
    state = track.TrackState(len(rows), n, curves_dev.device, ordered=True)
    row0 = 0
    for count in chunks or [len(rows)]:
        track.track_ordered_device(curves_dev, rows[row0:row0 + count], reach[row0:row0 + count], lams[row0:row0 + count], mu,
                                   back[row0:row0 + count], state, row0=row0, method=method)
        row0 += count
    assert row0 == len(rows)
    return state, track.track_ordered_backtrack_device(state)


def _host(curves, rows, weights, lams, mu, rs, back, n, method):
    kept = []
    want = track.track_ordered_host(track_cases.rows_of(curves, rows, n), weights, lams, mu, rs, back, method, _keep=kept)
    return want, kept[-1]


def _assert_equals_host(state, shifts, want, last_D):
    assert shifts.cpu().numpy().tolist() == want.shifts.tolist()
    row_min = state.row_min.cpu().numpy()
    assert (_bits64(row_min) == _bits64(want.row_min)).all() and _bits64(row_min[-1]) == _bits64(want.cost)
    assert state.row_arg.cpu().numpy().tolist() == want.row_arg.tolist()
    assert state.row_own_index.cpu().numpy().tolist() == want.row_own_index.tolist()
    assert (_bits(state.row_own_scores.cpu().numpy()) == _bits(want.row_own_scores)).all()
    assert (state.moves.cpu().numpy().reshape(want.moves.shape) == want.moves).all()
    assert (state.prefix_arg.cpu().numpy().reshape(want.prefix_arg.shape) == want.prefix_arg).all()
    assert (_bits64(state.last_D().cpu().numpy()) == _bits64(last_D)).all()
    # P of the last row is D at its jump sources
    assert (_bits64(state.P.cpu().numpy()) == _bits64(last_D[want.prefix_arg[-1]])).all()


# ---------------------------------------------------------------------------------------------- the pass, synthetic rows
@pytest.fixture(scope="module", params=METHODS)
def sequences(request):
    """One sequence per shape of cases.SHAPES, with track_ordered_host's answer: computed once."""
    out = {}
    for E, n, reach in cases.SHAPES:
        curves, rows, weights, lams, rs, mu, back = cases.sequence(E, n, reach, request.param, seed=3)
        out[(E, n, reach)] = (curves, rows, rs, lams, mu, back) + _host(curves, rows, weights, lams, mu, rs, back, n, request.param)
    return request.param, out


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_pass_equals_track_ordered_host(sequences, shape):
    """track_cases.SHAPES -- wave, workgroup and work-item edges, every halo size, rows at odd offsets, weights 1, 1/3, 0 and 2.5,
    equal minima at 511 | 512 and in the last element, an all-ones sequence -- with backs 0, 1, 255, 256, n - 1, n + 7 and no limit
    by turns and penalties 1, 1/4, 0, 2 and 1/2 times the sequence's by turns.  Shifts, cost, row_min, row_arg, the own extrema,
    every move, every jump source, the last D and its P: bitwise."""
    import torch
    method, table = sequences
    curves, rows, rs, lams, mu, back, want, last_D = table[shape]
    if shape[0] >= 7 and shape != (9, 65, 64):
        assert any(int(want.moves[e, want.shifts[e]]) == JUMP for e in range(1, shape[0]))
    state, shifts = _run(torch.from_numpy(curves).cuda(), rows, rs, lams, back, shape[1], mu, method)
    _assert_equals_host(state, shifts, want, last_D)
    assert state.back.cpu().numpy().tolist()[1:] == back[1:]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_small_axes(n, method):
    import torch
    for E, reach, seed in ((5, 1, 1), (8, 0, 2)):
        rng = np.random.default_rng(n * 31 + seed)
        lo = 0.25 if method == "sqdiff_normed" else -0.5
        curves = rng.random(E * (n + 2) + 3, dtype=np.float32) * np.float32(0.5) + np.float32(lo)
        rows = [(1 + e * (n + 2), (1.0, 1.0 / 3.0, 0.0, 2.5)[e % 4]) for e in range(E)]
        weights = [w for _o, w in rows]
        lams, back, rs = cases.penalties(E, 0.0625), cases.backs(E, n), [0] + [reach] * (E - 1)
        want, last_D = _host(curves, rows, weights, lams, track_cases.STEP_COST, rs, back, n, method)
        state, shifts = _run(torch.from_numpy(curves).cuda(), rows, rs, lams, back, n, track_cases.STEP_COST, method)
        _assert_equals_host(state, shifts, want, last_D)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("at", [256, 512])
def test_equal_minima_on_both_sides_of_a_boundary(at, method):
    """D_0's minimum twice, at at - 1 | at: the two sides of a scan round's boundary (256) and of a work item's (512): A is the lower
    index, and the jump just above the tie goes there."""
    import torch
    a, b = cases.prefix_tie_rows(1024, at, method)
    curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b])
    rows = [(1, 1.0), (1027, 1.0)]
    want, last_D = _host(curves, rows, [1.0, 1.0], [0.0, 0.0625], 0.0, [0, 0], [ANY, 0], 1024, method)
    assert want.prefix_arg[0, at] == at - 1 and want.prefix_arg[0, 1023] == at - 1 and want.moves[1, at + 1] == JUMP
    state, shifts = _run(torch.from_numpy(curves).cuda(), rows, [0, 0], [0.0, 0.0625], [ANY, 0], 1024, 0.0, method)
    _assert_equals_host(state, shifts, want, last_D)


@pytest.mark.parametrize("method", METHODS)
def test_pass_at_the_size_where_the_split_changes(method):
    """track_cases.PER_LARGE_FROM shifts: 1024 work items of 2048, eight scan rounds each, and four rounds of 256 records in the
    scan of the items.  Two rows, reach 2, back 256; row 0 falls from 0.75 to 0.25 in steps, so that records lie all along the axis."""
    import torch
    n, E = track_cases.PER_LARGE_FROM, 2
    rng = np.random.default_rng(23)
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    curves = np.empty(E * (n + 3) + 8, np.float32)
    rows = [(1 + e * (n + 3) + 2 * (e % 2), (1.0, 1.0 / 3.0)[e]) for e in range(E)]
    ramp = np.float32(0.75) - (np.arange(n) // 1000).astype(np.float32) * np.float32(0.5 / (n // 1000 + 1))
    curves[:] = np.float32(0.5) * sign
    curves[rows[0][0]:rows[0][0] + n] = (ramp + rng.random(n, dtype=np.float32) * np.float32(2.0 ** -12)) * sign
    curves[rows[1][0]:rows[1][0] + n] = (rng.random(n, dtype=np.float32) * np.float32(0.25) + np.float32(0.5)) * sign
    lams, back = [0.0, 2.0 ** -13], [ANY, 256]              # half a step of the ramp: a jump from the next step down pays
    want, last_D = _host(curves, rows, [w for _o, w in rows], lams, track_cases.STEP_COST, [0, 2], back, n, method)
    assert len(np.unique(want.prefix_arg[0])) > 1500 and np.count_nonzero(want.moves[1] == JUMP) > n // 8
    state, shifts = _run(torch.from_numpy(curves).cuda(), rows, [0, 2], lams, back, n, track_cases.STEP_COST, method)
    _assert_equals_host(state, shifts, want, last_D)


def test_a_sequence_in_chunks_has_the_bits_of_one_call(sequences):
    import torch
    method, table = sequences
    curves, rows, rs, lams, mu, back, want, last_D = table[(33, 1023, 127)]
    dev = torch.from_numpy(curves).cuda()
    whole, shifts = _run(dev, rows, rs, lams, back, 1023, mu, method)
    _assert_equals_host(whole, shifts, want, last_D)
    for chunks in ([1] * 33, [3] * 11, [2, 31]):
        parts, shifts_parts = _run(dev, rows, rs, lams, back, 1023, mu, method, chunks=chunks)
        assert torch.equal(shifts, shifts_parts)
        for a, b in zip(whole.tensors()[1:] + whole.order_tensors()[:2], parts.tensors()[1:] + parts.order_tensors()[:2]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert torch.equal(whole.last_D().view(torch.int64), parts.last_D().view(torch.int64))
        assert torch.equal(whole.back[1:], parts.back[1:])
    with pytest.raises(SushiError):
        track.track_ordered_device(dev, rows[:2], rs[:2], lams[:2], mu, back[:2], parts, row0=32, method=method)
    with pytest.raises(SushiError):
        track.track_ordered_device(dev, rows[1:3], rs[1:3], [0.5, -0.5], mu, back[1:3], parts, row0=1, method=method)
    with pytest.raises(SushiError):
        track.track_ordered_device(dev, rows[1:3], rs[1:3], lams[1:3], mu, [0, -2], parts, row0=1, method=method)
    with pytest.raises(SushiError):
        track.track_device(dev, rows[:2], rs[:2], 0.5, mu, parts, method=method)              # an ordered state, the plain call
    with pytest.raises(SushiError):
        track.track_ordered_device(dev, rows[:2], rs[:2], 0.5, mu, ANY, track.TrackState(33, 1023, dev.device), method=method)


def test_without_a_limit_it_is_todays_device_pass(sequences):
    """Every back without a limit and one penalty: every output the two passes share equals track_device + track_backtrack_device
    bitwise."""
    import torch
    method, _table = sequences
    for E, n, reach in ((33, 1023, 127), (16, 70001, 5), (7, 64, 3)):
        curves, rows, _weights, lam, rs, mu = track_cases.sequence(E, n, reach, method, seed=3)
        dev = torch.from_numpy(curves).cuda()
        ref = track.TrackState(E, n, dev.device)
        track.track_device(dev, rows, rs, lam, mu, ref, method=method)
        ref_shifts = track.track_backtrack_device(ref)
        for back in (ANY, [ANY] + [n - 1 + (e % 2) for e in range(1, E)]):
            got, shifts = _run(dev, rows, rs, [lam] * E, [back] * E if back == ANY else back, n, mu, method)
            assert torch.equal(shifts, ref_shifts)
            for a, b in zip(got.tensors()[1:], ref.tensors()[1:]):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            assert torch.equal(got.last_D().view(torch.int64), ref.last_D().view(torch.int64))
            assert torch.equal(got.prefix_arg.view(E, n)[:, n - 1], ref.row_arg)


# ---------------------------------------------------------------------------------------------- find_track(order=...)
@pytest.fixture(scope="module")
def decoys():
    dst, src = cases.streams()
    patterns, centres, bases = cases.scenario(dst, src)
    return dst, src, patterns, centres, bases


def _assert_track_equals(found, want, rows, k_lo, rate):
    assert [k - k_lo for k in found.shifts] == want.shifts.tolist() and _bits64(found.cost) == _bits64(want.cost)
    assert found.deltas == [k / float(rate) for k in found.shifts]
    assert [round(d * rate) - k_lo for d in found.event_own_delta] == want.row_own_index.tolist()
    assert (_bits(found.event_own_scores) == _bits(want.row_own_scores)).all()
    E = len(rows)
    jumps = [e for e in range(1, E) if want.moves[e, want.shifts[e]] == JUMP]
    assert found.jumps == jumps and found.moves == [0] + np.diff(want.shifts).tolist()
    assert found.segments == [(f, n, found.deltas[f], found.deltas[f + n - 1]) for f, n in track.jump_runs(E, jumps)]


@pytest.mark.parametrize("method", METHODS)
def test_find_track_in_order_on_the_decoy_scenario(decoys, method):
    """tests/test_track_order_host.py's scenario: at a penalty at which today's pass follows the decoys, find_track(order=True)
    returns the ten true shifts -- the host path's bits over match_templates rows, with and without clamp=0.5 under
    'ccoeff_normed' -- and find_track without order= still does what it did."""
    dst, _src, patterns, centres, bases = decoys
    rows = [r[0] for r in dst.match_templates(patterns, centres, [cases.WINDOW] * 10, method=method)]
    assert rows[0].shape[0] == cases.N_SHIFT
    back = track.order_back(bases, [p.shape[1] for p in patterns])
    want = track.track_ordered_host(rows, [1.0] * 10, cases.PENALTY, 0.0, 0, back, method)
    found = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, reach=0, order=True, method=method)
    assert (found.k_lo, found.n_shift) == (cases.K_LO, cases.N_SHIFT)
    _assert_track_equals(found, want, rows, cases.K_LO, cases.RATE)
    assert (_bits(found.event_scores) == _bits([r[s] for r, s in zip(rows, want.shifts)])).all()
    assert found.back == cases.BACK and found.penalties == [0.0] + [cases.PENALTY] * 9
    plain = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, reach=0, method=method)
    assert plain.back is None and plain.penalties is None
    _assert_track_equals(plain, track.track_host(rows, [1.0] * 10, cases.PENALTY, 0.0, 0, method), rows, cases.K_LO, cases.RATE)
    if method == "sqdiff_normed":
        assert found.shifts == cases.TRUE_K and found.jumps == [5] and plain.shifts == cases.RESULTS[cases.PENALTY][0]
        assert found.cost == cases.RESULTS[cases.PENALTY][3] and plain.cost == cases.RESULTS[cases.PENALTY][1]
        assert _bits(found.event_scores).tolist() == cases.EVENT_SCORE_BITS
        # backs given one by one, in three chunks, and a penalty per event alone
        listed = dst.find_track(patterns, centres, cases.WINDOW, [cases.PENALTY] * 10, reach=0, order=cases.BACK,
                                max_bytes=4 * 4 * cases.N_SHIFT + 3)
        assert listed.shifts == found.shifts and _bits64(listed.cost) == _bits64(found.cost) and listed.back == found.back
        lams = [0.0] + [0.01 if e == 5 else 1.0 for e in range(1, 10)]
        priced = dst.find_track(patterns, centres, cases.WINDOW, lams, reach=0)
        _assert_track_equals(priced, track.track_ordered_host(rows, [1.0] * 10, lams, 0.0, 0, ANY), rows, cases.K_LO, cases.RATE)
        assert priced.shifts == cases.TRUE_K and priced.back == [None] * 10 and priced.penalties == lams
        with pytest.raises(SushiError) as e:
            dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, reach=0, order=True, margins=True)
        assert "not built" in str(e.value)
    else:
        f = np.float32(0.5)
        clamped = [np.where(r >= f, r, f) for r in rows]
        want = track.track_ordered_host(clamped, [1.0] * 10, cases.PENALTY, 0.0, 0, back, method)
        got = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, reach=0, order=True, method=method, clamp=0.5)
        _assert_track_equals(got, want, clamped, cases.K_LO, cases.RATE)
        assert got.clamp == 0.5 and got.rows_info is not None
        assert (_bits(got.event_scores) == _bits([r[s] for r, s in zip(rows, want.shifts)])).all()       # the true scores


def test_calculate_tracked_shifts_in_order(decoys):
    dst, src, patterns, centres, _bases = decoys
    events = [ScriptEvent(s, e) for s, e in cases.EVENTS]
    got = calculate_tracked_shifts(src, dst, events, cases.WINDOW, cases.PENALTY, reach=0, order=True)
    assert got.shifts == cases.TRUE_K and got.jumps == [5] and got.back == cases.BACK
    for e, k, score in zip(events, cases.TRUE_K, got.event_scores):
        assert e.shift == k / float(cases.RATE) and _bits(e.diff) == _bits(score) and not e.linked
    plain = calculate_tracked_shifts(src, dst, events, cases.WINDOW, cases.PENALTY, reach=0)
    assert plain.shifts == cases.RESULTS[cases.PENALTY][0] and plain.back is None
    lams = [0.0] + [0.01 if e == 5 else 1.0 for e in range(1, 10)]
    priced = calculate_tracked_shifts(src, dst, events, cases.WINDOW, lams, reach=0)
    assert priced.shifts == cases.TRUE_K and priced.penalties == lams
