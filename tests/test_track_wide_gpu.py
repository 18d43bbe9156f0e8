"""Wide tracking on the GPU: sushi_hip_track_forward_wide / _wide_keep / sushi_hip_track_margins_wide against
their NumPy restatement (sushi_amd/track.py track_host / track_margins_host with wide=True), bit for bit down to the moves; rows of
a reach up to 1024 through the wide entry points against the plain entry points; chunks; two streams; find_track(wide=True), on the
long-gap scenario of tests/track_wide_cases.py end to end."""
import numpy as np
import pytest

import track_cases
import track_wide_cases as cases
from sushi_amd import synth, track
from sushi_amd.common import SushiError
from sushi_amd.wav import WavStream

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP = -32768
LAM = 0.0625                  # a jump costs more than most walks between the rows' values, and less than some


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(curves_dev, rows, reach, n, lam, mu, method, chunks=None, hip_stream=None, keep=False, forward=None):
    """The whole pass on the device through the wide entry points (or `forward`): forward calls over `chunks` (row counts;
    default: one call), then the backtrack."""
    state = track.TrackState(len(rows), n, curves_dev.device, keep=keep, wide=True)
    forward = forward or (track.track_wide_keep_device if keep else track.track_wide_device)
    row0 = 0
    for count in chunks or [len(rows)]:
        forward(curves_dev, rows[row0:row0 + count], reach[row0:row0 + count], lam, mu, state, row0=row0, method=method,
                hip_stream=hip_stream)
        row0 += count
    assert row0 == len(rows)
    return state, track.track_backtrack_device(state, hip_stream=hip_stream)


def _assert_equals_host(state, shifts, want):
    assert shifts.cpu().numpy().tolist() == want.shifts.tolist()
    row_min = state.row_min.cpu().numpy()
    assert (_bits64(row_min) == _bits64(want.row_min)).all() and _bits64(row_min[-1]) == _bits64(want.cost)
    assert state.row_arg.cpu().numpy().tolist() == want.row_arg.tolist()
    assert state.row_own_index.cpu().numpy().tolist() == want.row_own_index.tolist()
    assert (_bits(state.row_own_scores.cpu().numpy()) == _bits(want.row_own_scores)).all()
    assert (state.moves.cpu().numpy().reshape(want.moves.shape) == want.moves).all()


def _margins(curves_dev, rows, reach, guard, n, lam, mu, method, chunks=None, marginals=False, wide=True):
    import torch
    E = len(rows)
    state = track.TrackState(E, n, curves_dev.device, keep=True, wide=wide)
    forward, back = (track.track_wide_keep_device, track.track_wide_margins_device) if wide else \
        (track.track_forward_keep_device, track.track_margins_device)
    bounds = np.cumsum([0] + list(chunks or [E])).tolist()
    for a, b in zip(bounds[:-1], bounds[1:]):
        forward(curves_dev, rows[a:b], reach[a:b], lam, mu, state, row0=a, method=method)
    shifts = track.track_backtrack_device(state)
    M = torch.empty(E * n, dtype=torch.float64, device=curves_dev.device) if marginals else None
    for a, b in reversed(list(zip(bounds[:-1], bounds[1:]))):
        back(curves_dev, rows[a:b], reach[a:b + 1 if b < E else b], guard[a:b], lam, mu, state, shifts, row0=a, method=method, marginals=M)
    return state, shifts, M


def _assert_margins_equal_host(state, shifts, M, want):
    _assert_equals_host(state, shifts, want)
    assert (_bits64(state.D.cpu().numpy()) == _bits64(want.D.reshape(-1))).all()
    for name in ("through", "best", "alt", "c_min"):
        assert (_bits64(getattr(state, name).cpu().numpy()) == _bits64(getattr(want, name))).all(), name
    assert state.best_arg.cpu().numpy().tolist() == want.best_arg.tolist()
    assert state.alt_arg.cpu().numpy().tolist() == want.alt_arg.tolist()
    if M is not None:
        assert (_bits64(M.cpu().numpy()) == _bits64(want.marginals.reshape(-1))).all()


def _reaches(E, reach):
    return [0] + [reach] * (E - 1)


# ---------------------------------------------------------------------------------------------- forward + backtrack
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_wide_pass_equals_track_host(shape, method):
    """Rows at odd offsets, every kind of planted tie by turns, a free move of +0.0 and of -0.0: shifts, cost, row_min, row_arg, own
    extrema and every move, bitwise."""
    import torch
    E, n, reach = shape
    curves, rows, weights = cases.sequence(E, n, method, seed=5)
    assert all(o % 2 == 1 for o, _w in rows)
    dev = torch.from_numpy(curves).cuda()
    for mu in (0.0, -0.0):
        want = track.track_host(cases.rows_of(curves, rows, n), weights, LAM, mu, _reaches(E, reach), method, wide=True)
        _assert_equals_host(*_run(dev, rows, _reaches(E, reach), n, LAM, mu, method), want)
    words = want.moves[1:]
    assert (np.abs(words[words != JUMP]) > 1024).any() or n <= 1026       # moves no plain call could make


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_ties_across_a_work_item_boundary_and_at_both_ends(kind, method):
    """n = 4104 is eight work items of 512 and a bit, and four window tiles and a bit: the ties lie around the work-item boundary at
    2048 (also a tile boundary), around 2560 (a work-item boundary inside a tile) and at both axis ends."""
    import torch
    n = 4104
    for at in (2048, 2560):
        curves, rows, weights = cases.sequence(3, n, method, seed=2, kinds=(kind,), at=at)
        dev = torch.from_numpy(curves).cuda()
        for reach in (1025, 3000):
            want = track.track_host(cases.rows_of(curves, rows, n), weights, LAM, 0.0, _reaches(3, reach), method, wide=True)
            _assert_equals_host(*_run(dev, rows, _reaches(3, reach), n, LAM, 0.0, method), want)


@pytest.mark.parametrize("method", METHODS)
def test_mixed_reaches_chunks_and_two_streams(method):
    import torch
    E, n = 5, 4104
    curves, rows, weights = cases.sequence(E, n, method, seed=9)
    dev = torch.from_numpy(curves).cuda()
    want = track.track_host(cases.rows_of(curves, rows, n), weights, LAM, 0.0, cases.MIXED_REACH, method, wide=True)
    whole, shifts = _run(dev, rows, cases.MIXED_REACH, n, LAM, 0.0, method)
    _assert_equals_host(whole, shifts, want)
    for chunks in ([1, 2, 2], [2, 3]):               # a later call's row0 odd and even; a wide row first in its call
        parts, shifts_parts = _run(dev, rows, cases.MIXED_REACH, n, LAM, 0.0, method, chunks=chunks)
        assert torch.equal(shifts, shifts_parts)
        for a, b in zip(whole.tensors()[1:], parts.tensors()[1:]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert torch.equal(whole.last_D().view(torch.int64), parts.last_D().view(torch.int64))
    curves_b, rows_b, weights_b = cases.sequence(4, 32769, method, seed=4)
    dev_b = torch.from_numpy(curves_b).cuda()
    want_b = track.track_host(cases.rows_of(curves_b, rows_b, 32769), weights_b, LAM, 0.0, _reaches(4, 32767), method, wide=True)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, shifts_a = _run(dev, rows, cases.MIXED_REACH, n, LAM, 0.0, method, chunks=[2, 3], hip_stream=s1.cuda_stream)
    b, shifts_b = _run(dev_b, rows_b, _reaches(4, 32767), 32769, LAM, 0.0, method, hip_stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _assert_equals_host(a, shifts_a, want)
    _assert_equals_host(b, shifts_b, want_b)


@pytest.mark.parametrize("n", [track_cases.PER_LARGE_FROM, track_cases.PER_LARGE_FROM - 1])
def test_wide_pass_at_the_size_where_the_split_changes(n):
    """The shifts from which on a work item is 2048 indices, and one below it (items of 512 under a striding grid of 2048); three
    rows, reaches 1025 and 32767."""
    import torch
    curves, rows, weights = cases.sequence(3, n, "sqdiff_normed", seed=11, kinds=("random", "few_values", "runs"))
    reach = [0, 1025, 32767]
    want = track.track_host(cases.rows_of(curves, rows, n), weights, LAM, 0.0, reach, wide=True)
    _assert_equals_host(*_run(torch.from_numpy(curves).cuda(), rows, reach, n, LAM, 0.0, "sqdiff_normed"), want)


# ---------------------------------------------------------------------------------------------- narrow rows: the plain kernels
@pytest.mark.parametrize("method", METHODS)
def test_reaches_up_to_1024_through_the_wide_entry_points_are_the_plain_calls(method):
    import torch
    for E, n, reach in track_cases.SHAPES[3:6]:      # (9, 65, 64) (33, 1023, 127) (3, 4097, 1024)
        curves, rows, weights, lam, rs, mu = track_cases.sequence(E, n, reach, method, seed=3)
        dev = torch.from_numpy(curves).cuda()
        guard = [0, 120] * E
        for keep in (False, True):
            plain_forward = track.track_forward_keep_device if keep else track.track_device
            got, shifts = _run(dev, rows, rs, n, lam, mu, method, keep=keep)
            ref, ref_shifts = _run(dev, rows, rs, n, lam, mu, method, keep=keep, forward=plain_forward)
            assert torch.equal(shifts, ref_shifts)
            for a, b in zip(got.tensors()[1:], ref.tensors()[1:]):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            assert torch.equal(got.D.view(torch.int64), ref.D.view(torch.int64)) if keep else \
                torch.equal(got.last_D().view(torch.int64), ref.last_D().view(torch.int64))
        got, shifts, M = _margins(dev, rows, rs, guard[:E], n, lam, mu, method, marginals=True)
        ref, ref_shifts, ref_M = _margins(dev, rows, rs, guard[:E], n, lam, mu, method, marginals=True, wide=False)
        assert torch.equal(shifts, ref_shifts) and torch.equal(M.view(torch.int64), ref_M.view(torch.int64))
        for a, b in zip(got.margin_tensors()[1:], ref.margin_tensors()[1:]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---------------------------------------------------------------------------------------------- margins
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("guard", [0, 120])
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_wide_margins_equal_track_margins_host(shape, guard, method):
    """The forward test's shapes -- 70001 at reach 32767 is the axis longer than twice the reach, where a work item of the backward
    kernel stages 66 whole tiles' records from both sides -- with guard 0 and 120; M itself on one of them."""
    import torch
    E, n, reach = shape
    curves, rows, weights = cases.sequence(E, n, method, seed=6)
    dev = torch.from_numpy(curves).cuda()
    want = track.track_margins_host(cases.rows_of(curves, rows, n), weights, LAM, 0.0, _reaches(E, reach), guard, method, wide=True)
    marginals = shape == cases.SHAPES[1]
    state, shifts, M = _margins(dev, rows, _reaches(E, reach), [guard] * E, n, LAM, 0.0, method, marginals=marginals)
    _assert_margins_equal_host(state, shifts, M, want)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", cases.KINDS)
def test_wide_margins_on_ties_across_a_work_item_boundary_and_at_both_ends(kind, method):
    """The forward test's tie rows (n = 4104; ties around 2048 and 2560 and at both axis ends), backwards: guard 0 and 120."""
    import torch
    n = 4104
    for at, guard, reach in ((2048, 0, 1025), (2560, 120, 3000)):
        curves, rows, weights = cases.sequence(3, n, method, seed=2, kinds=(kind,), at=at)
        dev = torch.from_numpy(curves).cuda()
        want = track.track_margins_host(cases.rows_of(curves, rows, n), weights, LAM, 0.0, _reaches(3, reach), guard, method, wide=True)
        state, shifts, M = _margins(dev, rows, _reaches(3, reach), [guard] * 3, n, LAM, 0.0, method, marginals=True)
        _assert_margins_equal_host(state, shifts, M, want)


@pytest.mark.parametrize("n", [track_cases.PER_LARGE_FROM, track_cases.PER_LARGE_FROM - 1])
def test_wide_margins_at_the_size_where_the_split_changes(n):
    import torch
    curves, rows, weights = cases.sequence(3, n, "sqdiff_normed", seed=11, kinds=("random", "few_values", "runs"))
    reach = [0, 1025, 32767]
    want = track.track_margins_host(cases.rows_of(curves, rows, n), weights, LAM, 0.0, reach, [0, 120, 0], wide=True)
    state, shifts, M = _margins(torch.from_numpy(curves).cuda(), rows, reach, [0, 120, 0], n, LAM, 0.0, "sqdiff_normed")
    _assert_margins_equal_host(state, shifts, M, want)


@pytest.mark.parametrize("method", METHODS)
def test_wide_margins_mixed_reaches_in_chunks(method):
    import torch
    E, n = 5, 4104
    curves, rows, weights = cases.sequence(E, n, method, seed=9)
    dev = torch.from_numpy(curves).cuda()
    want = track.track_margins_host(cases.rows_of(curves, rows, n), weights, LAM, -0.0, cases.MIXED_REACH, [0, 120, 7, 0, 5000], method,
                                    wide=True)
    for chunks in (None, [1, 2, 2], [2, 3]):
        state, shifts, M = _margins(dev, rows, cases.MIXED_REACH, [0, 120, 7, 0, 5000], n, LAM, -0.0, method, chunks=chunks,
                                    marginals=True)
        _assert_margins_equal_host(state, shifts, M, want)


# ---------------------------------------------------------------------------------------------- refusals, find_track
def test_wide_device_calls_refuse_on_the_host():
    import torch
    curves, rows, _weights = cases.sequence(3, 1100, "sqdiff_normed")
    dev = torch.from_numpy(curves).cuda()
    state = track.TrackState(3, 1100, dev.device, wide=True)
    with pytest.raises(SushiError) as e:
        track.track_wide_device(dev, rows, [0, 32768, 5], LAM, 0.0, state)
    assert "event 1" in str(e.value) and "32768" in str(e.value) and "32767" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.track_wide_device(dev, rows, [0, 5, 1025], LAM, 0.25, state)
    assert "event 2" in str(e.value) and "1025" in str(e.value) and "0.25" in str(e.value)
    with pytest.raises(SushiError):
        track.track_device(dev, rows, [0, 5, 1025], LAM, 0.0, state)            # the plain call keeps its bound
    with pytest.raises(SushiError):
        track.TrackState(3, 1100, dev.device, ordered=True, wide=True)


@pytest.fixture(scope="module")
def wander(oracle):
    dst, src = track_cases.streams()
    patterns, centres, bases = track_cases.scenario(dst, src)
    rows = track_cases.oracle_rows(oracle, dst, patterns, bases, track_cases.K_LO, track_cases.N_SHIFT)
    return dst, src, patterns, centres, rows


WIDE_REACH = [0, 88, 1025, 81, 102, 6000, 88, 32767, 88, 88]


def _assert_track_equals(found, want, rows, k_lo):
    assert [k - k_lo for k in found.shifts] == want.shifts.tolist() and _bits64(found.cost) == _bits64(want.cost)
    assert (_bits(found.event_scores) == _bits([r[s] for r, s in zip(rows, want.shifts)])).all()
    assert (_bits(found.event_own_scores) == _bits(want.row_own_scores)).all()
    jumps = [e for e in range(1, len(rows)) if want.moves[e, want.shifts[e]] == JUMP]
    assert found.jumps == jumps and found.moves == [0] + np.diff(want.shifts).tolist()


def test_find_track_wide_on_the_wandering_shift_scenario(wander):
    """tests/track_cases.py's ten uint8 events with reaches that pass 1024 in three rows, one of them wide enough to walk the cut
    (5400 samples): against track_host(wide=True) over the CPU oracle's rows -- plain, with margins, clamped and in chunks."""
    dst, _src, patterns, centres, rows = wander
    K, N, lam = track_cases.K_LO, track_cases.N_SHIFT, track_cases.PENALTY
    want = track.track_margins_host(rows, [1.0] * 10, lam, 0.0, WIDE_REACH, 120, wide=True)
    words = [int(want.moves[e, want.shifts[e]]) for e in range(1, 10)]
    assert any(w != JUMP and abs(w) > 1024 for w in words)                          # a move no plain call could make
    found = dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=WIDE_REACH, wide=True)
    _assert_track_equals(found, want, rows, K)
    assert found.reach == WIDE_REACH and found.event_margin is None
    with_margins = dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=WIDE_REACH, wide=True, margins=True, guard=120,
                                  marginals=True)
    _assert_track_equals(with_margins, want, rows, K)
    assert (_bits64(with_margins.event_through) == _bits64(want.through)).all()
    assert (_bits64(with_margins.marginals.cpu().numpy()) == _bits64(want.marginals)).all()
    assert [None if k is None else k - K for k in with_margins.event_alt_shift] == [None if k < 0 else k for k in want.alt_arg.tolist()]
    chunked = dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=WIDE_REACH, wide=True, margins=True, guard=120,
                             max_bytes=4 * 3 * N + 3)                               # 3 + 3 + 3 + 1 events
    assert chunked.shifts == found.shifts and _bits64(chunked.cost) == _bits64(found.cost)
    assert (_bits64(chunked.event_through) == _bits64(with_margins.event_through)).all()
    assert (_bits64(chunked.event_margin) == _bits64(with_margins.event_margin)).all()
    f = 0.5
    clamped_rows = [np.minimum(r, np.float32(f)) for r in rows]
    clamped = dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=WIDE_REACH, wide=True, clamp=f)
    want_c = track.track_host(clamped_rows, [1.0] * 10, lam, 0.0, WIDE_REACH, wide=True)
    assert [k - K for k in clamped.shifts] == want_c.shifts.tolist() and _bits64(clamped.cost) == _bits64(want_c.cost)
    # without wide= the call ends as before; with it, the remaining refusals
    with pytest.raises(SushiError) as e:
        dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=WIDE_REACH)
    assert "event 2" in str(e.value) and "1025" in str(e.value) and "1024" in str(e.value)
    need = track.TrackState.nbytes(10, N, wide=True)
    assert need == track.TrackState.nbytes(10, N) + track.wide_workspace_bytes(N)
    with pytest.raises(SushiError) as e:
        dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=WIDE_REACH, wide=True, max_state_bytes=need - 1)
    assert str(need) in str(e.value)
    with pytest.raises(SushiError) as e:
        dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=WIDE_REACH, wide=True, step_cost=1e-3)
    assert "event 2" in str(e.value) and "1025" in str(e.value) and "0.001" in str(e.value)
    with pytest.raises(SushiError) as e:
        dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=[0] + [32768] * 9, wide=True)
    assert "32768" in str(e.value) and "32767" in str(e.value)
    for kw in (dict(order=True), dict(order=[None] * 10)):
        with pytest.raises(SushiError) as e:
            dst.find_track(patterns, centres, track_cases.WINDOW, lam, reach=WIDE_REACH, wide=True, **kw)
        assert "1024" in str(e.value) and "ordered" in str(e.value)
    with pytest.raises(SushiError):
        dst.find_track(patterns, centres, track_cases.WINDOW, [lam] * 10, reach=WIDE_REACH, wide=True)
    with pytest.raises(SushiError):
        dst.find_ordered_track(patterns, centres, track_cases.WINDOW, lam, reach=88, wide=True)


def test_find_track_wide_f32_equals_track_host_over_match_templates():
    rate = 12000
    dst_pcm = synth.make_dst_pcm(12, rate, seed=31)
    src_pcm = synth.make_src_pcm(dst_pcm, [(0, 1500), (37000, 1530), (60000, -900), (82000, -925)], seed=32)
    dst, src = (WavStream.from_samples(p, rate, sample_type='float32') for p in (dst_pcm, src_pcm))
    spans = [(2.0, 2.5), (3.25, 3.75), (6.0, 6.625), (7.5, 7.875)]
    patterns, centres = [src.get_substream(s, e) for s, e in spans], [s for s, _e in spans]
    rows = [r[0] for r in dst.match_templates(patterns, centres, [0.5] * 4)]
    reach = track.rate_reach([dst._get_sample_for_time(c) for c in centres], 0.075)
    assert reach[0] == 0 and min(reach[1:]) > 1024 and max(reach) <= 32767
    want = track.track_host(rows, [1.0] * 4, 0.25, 0.0, reach, wide=True)
    got = dst.find_track(patterns, centres, 0.5, 0.25, max_rate=0.075, wide=True)
    _assert_track_equals(got, want, rows, got.k_lo)
    assert got.reach == reach and got.n_shift == rows[0].shape[0]


# ---------------------------------------------------------------------------------------------- the long-gap scenario
@pytest.fixture(scope="module")
def gap(oracle):
    """tests/track_wide_cases.py's long-gap scenario with event 5's decoy planted, and the CPU oracle's rows of it."""
    dst, src = cases.gap_streams(decoy=True)
    patterns, centres, bases = cases.gap_scenario(dst, src)
    rows = track_cases.oracle_rows(oracle, dst, patterns, bases, cases.GAP_K_LO, cases.GAP_N_SHIFT)
    return dst, src, patterns, centres, rows


def test_find_track_wide_walks_the_long_gap(gap):
    """tests/test_track_wide_host.py's scenario end to end, uint8 streams: max_rate 9e-3 gives event 5 a reach of 2399.  Without
    wide= the call ends; with the reaches clipped to 1024 by hand it lands on event 5's decoy and pays a jump one event later; with
    wide=True it returns the ten true shifts and no jump, at every penalty of cases.GAP_PENALTIES -- each against
    track_host over the oracle's rows, bit for bit; also with margins, clamped, and in chunks."""
    dst, _src, patterns, centres, rows = gap
    K, N = cases.GAP_K_LO, cases.GAP_N_SHIFT
    with pytest.raises(SushiError) as e:
        dst.find_track(patterns, centres, cases.GAP_WINDOW, 0.5, max_rate=cases.GAP_MAX_RATE)
    assert "event 5" in str(e.value) and "2399" in str(e.value) and "1024" in str(e.value)
    clipped = dst.find_track(patterns, centres, cases.GAP_WINDOW, 0.5, reach=cases.GAP_CLIPPED)
    assert clipped.shifts == cases.GAP_DECOY_K and clipped.jumps == [6]
    _assert_track_equals(clipped, track.track_host(rows, [1.0] * 10, 0.5, 0.0, cases.GAP_CLIPPED), rows, K)
    for lam in cases.GAP_PENALTIES:
        found = dst.find_track(patterns, centres, cases.GAP_WINDOW, lam, max_rate=cases.GAP_MAX_RATE, wide=True)
        assert (found.k_lo, found.n_shift, found.reach) == (K, N, cases.GAP_REACH)
        assert found.shifts == cases.GAP_TRUE_K and found.jumps == [] and found.moves[5] == -1890
        _assert_track_equals(found, track.track_host(rows, [1.0] * 10, lam, 0.0, cases.GAP_REACH, wide=True), rows, K)
    assert found.cost < clipped.cost
    for lam in cases.GAP_PENALTIES_BELOW_THE_NOISE[-1:]:                            # below the noise's price the decoy wins, wide or not
        low = dst.find_track(patterns, centres, cases.GAP_WINDOW, lam, max_rate=cases.GAP_MAX_RATE, wide=True)
        assert low.shifts == cases.GAP_DECOY_K and low.jumps == [6]
    want = track.track_margins_host(rows, [1.0] * 10, 0.5, 0.0, cases.GAP_REACH, 120, wide=True)
    for kw in (dict(), dict(max_bytes=4 * 3 * N + 3)):                              # one chunk; 3 + 3 + 3 + 1 events
        m = dst.find_track(patterns, centres, cases.GAP_WINDOW, 0.5, max_rate=cases.GAP_MAX_RATE, wide=True, margins=True, guard=120,
                           marginals=True, **kw)
        _assert_track_equals(m, want, rows, K)
        assert (_bits64(m.event_through) == _bits64(want.through)).all()
        assert (_bits64(m.marginals.cpu().numpy()) == _bits64(want.marginals)).all()
        assert m.event_alt_shift[5] == cases.GAP_DECOY_K[5] and m.event_margin[5] > 0.3      # event 5's best alternative is its decoy
    f = 0.5
    clamped = dst.find_track(patterns, centres, cases.GAP_WINDOW, 0.5, max_rate=cases.GAP_MAX_RATE, wide=True, clamp=f)
    want_c = track.track_host([np.minimum(r, np.float32(f)) for r in rows], [1.0] * 10, 0.5, 0.0, cases.GAP_REACH, wide=True)
    assert clamped.shifts == cases.GAP_TRUE_K and _bits64(clamped.cost) == _bits64(want_c.cost)


def test_find_track_wide_walks_the_long_gap_in_float32_streams():
    """The same scenario in float32 streams, against track_host over the events' score curves on the joint axis (match_curves:
    exact per position; match_templates rounds every event's window for itself, so its rows do not share an axis)."""
    from sushi_amd import axis
    from sushi_amd.curves import match_curves
    dst, src = cases.gap_streams(decoy=True, sample_type='float32')
    patterns, centres, _bases = cases.gap_scenario(dst, src)
    dst_dev = dst.device_stream()
    src_dev, offs, lens, _ = dst._pattern_source(patterns, dst_dev)
    lens = axis.pattern_lengths(lens)
    ax = axis.event_axis(dst, offs, lens, centres, cases.GAP_WINDOW)
    assert (ax.k_lo, ax.n_shift) == (cases.GAP_K_LO, cases.GAP_N_SHIFT)
    curves, at = match_curves(dst_dev, src_dev, ax.offs, lens, [b + ax.k_lo for b in ax.bases], [ax.n_shift] * 10)
    curves = curves.cpu().numpy()
    rows = [curves[at[k]:at[k + 1]] for k in range(10)]
    found = dst.find_track(patterns, centres, cases.GAP_WINDOW, 0.5, max_rate=cases.GAP_MAX_RATE, wide=True)
    _assert_track_equals(found, track.track_host(rows, [1.0] * 10, 0.5, 0.0, cases.GAP_REACH, wide=True), rows, cases.GAP_K_LO)
    assert found.shifts == cases.GAP_TRUE_K and found.jumps == [] and found.reach == cases.GAP_REACH
    clipped = dst.find_track(patterns, centres, cases.GAP_WINDOW, 0.5, reach=cases.GAP_CLIPPED)
    _assert_track_equals(clipped, track.track_host(rows, [1.0] * 10, 0.5, 0.0, cases.GAP_CLIPPED), rows, cases.GAP_K_LO)
    assert clipped.shifts == cases.GAP_DECOY_K and clipped.jumps == [6]
