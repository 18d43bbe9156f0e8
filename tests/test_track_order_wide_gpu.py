"""Wide ordered tracking on the GPU: sushi_hip_track_forward_ordered_wide / _wide_keep + the ordered backtrack and
sushi_hip_track_order_margins_wide against their NumPy restatement (sushi_amd/track.py track_ordered_margins_host(wide=True)), bit
for bit down to every D, move word, A, M, the two halves of C, P and S: axes of one, two and four window tiles and a bit, a reach
wider than the axis, the widest reach on an axis just above it and on one longer than twice it; backs and penalties that vary by
row; ties across a work item's boundary and at both ends; equal minima of the prefix on both sides of a wave's and a work item's
boundary in front of a wide row; the size where the work split changes; mixed reaches; chunks whose first row is wide; two streams;
guards; the ordered calls where no reach passes 1024 and the plain wide calls where no back binds;
WavStream.find_ordered_wide_track on the scenario that needs both."""
import numpy as np
import pytest

import track_cases
import track_order_cases as ocases
import track_order_wide_cases as cases
import track_wide_cases as wcases
from sushi_amd import track
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, calculate_ordered_wide_shifts

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")
JUMP, ANY = -32768, -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _forward(dev, rows, reach, lams, back, n, mu, method, chunks=None, keep=True, stream=None, wide=True):
    """The wide ordered forward pass (keep: with its rows kept) over `chunks` (row counts; default: one call), then the backtrack."""
    state = track.TrackState(len(rows), n, dev.device, ordered=True, margins=keep)
    if wide:
        call = track.track_ordered_wide_keep_device if keep else track.track_ordered_wide_device
    else:
        call = track.track_ordered_keep_device if keep else track.track_ordered_device
    row0 = 0
    for count in chunks or [len(rows)]:
        call(dev, rows[row0:row0 + count], reach[row0:row0 + count], lams[row0:row0 + count], mu, back[row0:row0 + count], state,
             row0=row0, method=method, hip_stream=stream)
        row0 += count
    assert row0 == len(rows)
    return state, track.track_ordered_backtrack_device(state, hip_stream=stream)


def _margins(dev, rows, reach, lams, back, guard, mu, method, state, shifts, chunks=None, marginals=True, stream=None, wide=True):
    """The backward walk over `chunks` (row counts from the last row down; default: one call) -> M as [E, n] (or None)."""
    import torch
    E, n = len(rows), state.n_shift
    M = torch.full((E * n,), float("nan"), dtype=torch.float64, device=dev.device) if marginals else None
    call = track.track_ordered_wide_margins_device if wide else track.track_ordered_margins_device
    last = E
    for count in chunks or [E]:
        first = last - count
        upto = last + 1 if last < E else last
        call(dev, rows[first:last], reach[first:upto], guard[first:last], lams[first:upto], mu, back[first:upto], state, shifts,
             row0=first, method=method, marginals=M, hip_stream=stream)
        last = first
    assert last == 0
    return None if M is None else M.view(E, n)


def _host(curves, rows, weights, lams, mu, rs, back, guard, n, method):
    trace = []
    want = track.track_ordered_margins_host(cases.rows_of(curves, rows, n), weights, lams, mu, rs, back, guard, method, _trace=trace,
                                            wide=True)
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
    if state.margins:
        assert (_bits64(state.D.cpu().numpy().reshape(want.D.shape)) == _bits64(want.D)).all()      # every row of D
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


def _whole(curves, rows, weights, lams, mu, rs, back, guard, n, method, chunks=None, back_chunks=None, marginals=True):
    """Forward with the rows kept, backtrack and margins on the device against the host: everything, bitwise; and the forward call
    that keeps no rows against the one that does."""
    import torch
    want, by_row = _host(curves, rows, weights, lams, mu, rs, back, guard, n, method)
    dev = torch.from_numpy(curves).cuda()
    state, shifts = _forward(dev, rows, rs, lams, back, n, mu, method, chunks=chunks)
    _assert_forward_equals_host(state, shifts, want)
    lean, lean_shifts = _forward(dev, rows, rs, lams, back, n, mu, method, chunks=chunks, keep=False)
    _assert_forward_equals_host(lean, lean_shifts, want)
    M = _margins(dev, rows, rs, lams, back, guard, mu, method, state, shifts, chunks=back_chunks, marginals=marginals)
    _assert_margins_equal_host(state, M, want, by_row)
    return want


# ---------------------------------------------------------------------------------------------- the passes, synthetic rows
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_forward_backtrack_and_margins_equal_the_host(shape, method):
    """(E, n, reach) of track_wide_cases.SHAPES -- 1025 on axes of one tile and two values, of two and of four tiles and a bit; a
    reach wider than the axis; 32767 on an axis just above it and on 70001 shifts, where a work item stages 66 whole tiles' records
    from both sides -- every kind of planted tie, backs 0, 1, 255, 256, n - 1, n + 7 and none by turns, penalties and guards per
    row, marginals=True."""
    E, n, reach = shape
    curves, rows, weights, lams, rs, back, guard = cases.sequence(E, n, reach, method, seed=6)
    _whole(curves, rows, weights, lams, (0.0, -0.0)[n % 2], rs, back, guard, n, method)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("guard", [0, 120])
def test_every_back_on_a_wide_row_and_both_guards(guard, method):
    """Eight rows over 4104 shifts, so that every back of track_order_cases.backs -- 0, 1, 255, 256, n - 1, n + 7, none -- meets a
    wide row, reach 1025 and 3000 by turns; one guard for every row."""
    E, n = 8, 4104
    curves, rows, weights, lams, rs, back, _g = cases.sequence(E, n, [0] + [(1025, 3000)[e % 2] for e in range(1, E)], method, seed=4)
    assert sorted(set(back[1:])) == sorted({0, 1, 255, 256, n - 1, n + 7, ANY})
    _whole(curves, rows, weights, lams, 0.0, rs, back, [guard] * E, n, method, marginals=False)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("kind", wcases.KINDS)
def test_ties_across_a_work_item_boundary_and_at_both_ends(kind, method):
    """Tie rows of one kind (n = 4104: work items of 2048) with the ties around 2048 -- a work item's boundary, and a window tile's --
    and around 2560, and the kinds' own ties at both axis ends; back 256 and none."""
    n = 4104
    for at, reach in ((2048, 1025), (2560, 3000)):
        curves, rows, weights, lams, rs, _back, guard = cases.sequence(3, n, reach, method, seed=2, kinds=(kind,), at=at)
        _whole(curves, rows, weights, lams, 0.0, rs, [ANY, 256, ANY], guard, n, method)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("at", [256, 512])
def test_equal_prefix_minima_on_both_sides_of_a_boundary_in_front_of_a_wide_row(at, method):
    """track_order_cases.prefix_tie_rows: row 0's minimum twice, at at - 1 | at -- the two sides of a wave's and a round's boundary
    (255 | 256) and of a work item's (511 | 512) -- followed by a wide row that reads P and A there: t_e lands on each side with
    back 0, 1, `at` and none.  (On 1100 shifts a work item is 512 indices.)"""
    n = 1100
    a, b = ocases.prefix_tie_rows(n, at, method)
    curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b, np.zeros(1, np.float32), a[::-1]])
    rows = [(1, 1.0), (n + 3, 1.0), (2 * n + 4, 1.0)]
    for back in (0, 1, at, ANY):
        want = _whole(curves, rows, [1.0] * 3, [0.0, 0.0625, 0.0625], 0.0, [0, 1025, 1099], [ANY, back, back], [0, 5, 300], n, method)
        assert abs(want.row_min[0]) == 0.25 and want.prefix_arg[0, at - 1] == at - 1 and want.prefix_arg[0, at] == at - 1


@pytest.mark.parametrize("n", [track_cases.PER_LARGE_FROM, track_cases.PER_LARGE_FROM - 1])
def test_at_the_size_where_the_split_changes(n):
    """track_cases.PER_LARGE_FROM shifts: work items of 2048 (eight indices a thread); one shift fewer: items of 512."""
    curves, rows, weights, lams, _rs, _back, _g = cases.sequence(3, n, 0, "sqdiff_normed", seed=11, kinds=("random", "few_values", "runs"))
    _whole(curves, rows, weights, lams, 0.0, [0, 1025, 32767], [ANY, 256, n + 7], [0, 120, 0], n, "sqdiff_normed", marginals=False)


@pytest.mark.parametrize("method", METHODS)
def test_mixed_reaches_chunks_and_two_streams(method):
    """Reaches [0, 7, 1025, 64, 3000].  Chunks with an odd and an even row0 whose first row is wide -- forward it reads P and D left
    in the state (rows 2 and 4 after [2, 2, 1]; row 2 after [2, 3]), backward it reads S and C (the calls that end at rows 1 and 3:
    the steps into rows 2 and 4 are the wide ones) -- and the same sequence on two streams at once."""
    import torch
    E, n = 5, 4104
    curves, rows, weights, lams, rs, back, guard = cases.sequence(E, n, cases.MIXED_REACH, method, seed=9)
    want, by_row = _host(curves, rows, weights, lams, -0.0, rs, back, guard, n, method)
    dev = torch.from_numpy(curves).cuda()
    for chunks, back_chunks in ((None, None), ([2, 2, 1], [1, 2, 2]), ([2, 3], [3, 2]), ([1, 1, 1, 1, 1], [1] * 5), ([4, 1], [2, 3])):
        state, shifts = _forward(dev, rows, rs, lams, back, n, -0.0, method, chunks=chunks)
        _assert_forward_equals_host(state, shifts, want)
        M = _margins(dev, rows, rs, lams, back, guard, -0.0, method, state, shifts, chunks=back_chunks)
        _assert_margins_equal_host(state, M, want, by_row)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    done = []
    for st in streams:
        with torch.cuda.stream(st):
            state, shifts = _forward(dev, rows, rs, lams, back, n, -0.0, method, chunks=[2, 3], stream=st.cuda_stream)
            done.append((state, shifts, _margins(dev, rows, rs, lams, back, guard, -0.0, method, state, shifts, chunks=[3, 2],
                                                 stream=st.cuda_stream)))
    torch.cuda.synchronize()
    for state, shifts, M in done:
        _assert_forward_equals_host(state, shifts, want)
        _assert_margins_equal_host(state, M, want, by_row)


# ---------------------------------------------------------------------------------------------- the two equivalences
@pytest.mark.parametrize("method", METHODS)
def test_reaches_up_to_1024_through_the_wide_entry_points_are_the_ordered_calls(method):
    import torch
    for E, n, reach in track_cases.SHAPES[3:6]:      # (9, 65, 64) (33, 1023, 127) (3, 4097, 1024)
        curves, rows, _weights, lams, rs, mu, back = ocases.sequence(E, n, reach, method, seed=3)
        lams = [0.0] + lams[1:]
        guard = cases.guards(E, n)
        dev = torch.from_numpy(curves).cuda()
        for keep in (False, True):
            got, shifts = _forward(dev, rows, rs, lams, back, n, mu, method, keep=keep)
            ref, ref_shifts = _forward(dev, rows, rs, lams, back, n, mu, method, keep=keep, wide=False)
            assert torch.equal(shifts, ref_shifts)
            for a, b in zip(got.tensors()[1:] + got.order_tensors(), ref.tensors()[1:] + ref.order_tensors()):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
            assert torch.equal(got.D.view(torch.int64), ref.D.view(torch.int64)) if keep else \
                torch.equal(got.last_D().view(torch.int64), ref.last_D().view(torch.int64))
        M = _margins(dev, rows, rs, lams, back, guard, mu, method, got, shifts)
        ref_M = _margins(dev, rows, rs, lams, back, guard, mu, method, ref, ref_shifts, wide=False)
        assert torch.equal(M.view(torch.int64), ref_M.view(torch.int64))
        for a, b in zip(got.margin_tensors() + (got.S,), ref.margin_tensors() + (ref.S,)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("method", METHODS)
def test_without_a_limit_they_are_the_plain_wide_calls(method):
    """Every back without a limit (or >= n_shift - 1) and one penalty: every output the calls share equals track_wide_keep_device +
    track_backtrack_device + track_wide_margins_device bitwise."""
    import torch
    for (E, n, reach), back in (((5, 4104, cases.MIXED_REACH), ANY), ((4, 32769, 32767), [ANY, 32768, 40000, ANY])):
        curves, rows, _weights = wcases.sequence(E, n, method, seed=6)
        rs = [0] + ([reach] * (E - 1) if np.ndim(reach) == 0 else list(reach)[1:])
        guard = cases.guards(E, n)
        dev = torch.from_numpy(curves).cuda()
        ref = track.TrackState(E, n, dev.device, keep=True)
        track.track_wide_keep_device(dev, rows, rs, cases.LAM, 0.0, ref, method=method)
        ref_shifts = track.track_backtrack_device(ref)
        ref_M = torch.empty(E * n, dtype=torch.float64, device=dev.device)
        track.track_wide_margins_device(dev, rows, rs, guard, cases.LAM, 0.0, ref, ref_shifts, method=method, marginals=ref_M)
        backs = [back] * E if np.ndim(back) == 0 else back
        got, shifts = _forward(dev, rows, rs, [cases.LAM] * E, backs, n, 0.0, method)
        M = _margins(dev, rows, rs, [cases.LAM] * E, backs, guard, 0.0, method, got, shifts)
        assert torch.equal(shifts, ref_shifts) and torch.equal(M.reshape(-1).view(torch.int64), ref_M.view(torch.int64))
        for a, b in zip(got.tensors() + got.margin_tensors(), ref.tensors() + ref.margin_tensors()):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---------------------------------------------------------------------------------------------- refusals, end to end
def test_device_calls_refuse_on_the_host():
    import torch
    curves, rows, _weights = wcases.sequence(3, 1100, "sqdiff_normed")
    dev = torch.from_numpy(curves).cuda()
    state = track.TrackState(3, 1100, dev.device, ordered=True)
    kept = track.TrackState(3, 1100, dev.device, ordered=True, margins=True)
    with pytest.raises(SushiError) as e:
        track.track_ordered_wide_device(dev, rows, [0, 32768, 5], cases.LAM, 0.0, ANY, state)
    assert "event 1" in str(e.value) and "32768" in str(e.value) and "32767" in str(e.value)
    with pytest.raises(SushiError) as e:
        track.track_ordered_wide_device(dev, rows, [0, 5, 1025], cases.LAM, 0.25, ANY, state)
    assert "event 2" in str(e.value) and "1025" in str(e.value) and "0.25" in str(e.value)
    with pytest.raises(SushiError):
        track.track_ordered_device(dev, rows, [0, 5, 1025], cases.LAM, 0.0, ANY, state)          # the ordered call keeps its bound
    with pytest.raises(SushiError):
        track.track_ordered_wide_device(dev, rows, [0, 5, 1025], cases.LAM, 0.0, ANY, kept)      # a state that keeps its rows
    with pytest.raises(SushiError):
        track.track_ordered_wide_keep_device(dev, rows, [0, 5, 1025], cases.LAM, 0.0, ANY, state)
    with pytest.raises(SushiError):
        track.track_ordered_wide_device(dev, rows, [0, 5, 1025], cases.LAM, 0.0, ANY, track.TrackState(3, 1100, dev.device))
    shifts = torch.zeros(3, dtype=torch.int32, device=dev.device)
    with pytest.raises(SushiError) as e:
        track.track_ordered_wide_margins_device(dev, rows, [0, 5, 1025], 0, cases.LAM, 0.25, ANY, kept, shifts)
    assert "event 2" in str(e.value) and "1025" in str(e.value)
    with pytest.raises(SushiError):
        track.track_ordered_wide_margins_device(dev, rows, [0, 5, 1025], 0, cases.LAM, 0.0, ANY, state, shifts)
    with pytest.raises(SushiError):
        track.TrackState(3, 1100, dev.device, ordered=True, wide=True)                          # the old refusal stands


@pytest.fixture(scope="module")
def both(oracle):
    """tests/track_order_wide_cases.py's scenario and the CPU oracle's rows of it."""
    dst, src = cases.streams()
    patterns, centres, bases = cases.scenario(dst, src)
    rows = track_cases.oracle_rows(oracle, dst, patterns, bases, cases.K_LO, cases.N_SHIFT)
    return dst, src, patterns, centres, rows


def _assert_track_equals(found, want, rows, k_lo):
    assert [k - k_lo for k in found.shifts] == want.shifts.tolist() and _bits64(found.cost) == _bits64(want.cost)
    assert (_bits(found.event_scores) == _bits([r[s] for r, s in zip(rows, want.shifts)])).all()
    assert (_bits(found.event_own_scores) == _bits(want.row_own_scores)).all()
    jumps = [e for e in range(1, len(rows)) if want.moves[e, want.shifts[e]] == JUMP]
    assert found.jumps == jumps and found.moves == [0] + np.diff(want.shifts).tolist()


def test_find_ordered_wide_track_needs_both_at_once(both):
    """The scenario end to end, uint8 streams: conditions (a) - (d) of tests/track_order_wide_cases.py on the device, each call
    against its host restatement over the oracle's rows bit for bit; with margins, marginals, in chunks and clamped."""
    dst, src, patterns, centres, rows = both
    K, N, w = cases.K_LO, cases.N_SHIFT, [1.0] * 10
    back = [ANY] + cases.BACK[1:]
    for lam in cases.PENALTIES:
        # (a) the plain wide pass follows both decoys; the wide ordered pass does not, and walks into event 5
        plain = dst.find_track(patterns, centres, cases.WINDOW, lam, max_rate=cases.MAX_RATE, wide=True)
        assert plain.shifts == cases.DECOYED_K and plain.jumps == cases.DECOYED_JUMPS
        found = dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, lam, order=True, max_rate=cases.MAX_RATE)
        assert (found.k_lo, found.n_shift, found.reach, found.back) == (K, N, cases.REACH, cases.BACK)
        assert found.shifts == cases.TRUE_K and found.jumps == [] and found.moves[5] == -1890
        want = track.track_ordered_host(rows, w, lam, 0.0, cases.REACH, back, wide=True)
        _assert_track_equals(found, want, rows, K)
        assert abs(found.cost - cases.RESULTS[lam][1]) < 1e-12 and abs(plain.cost - cases.RESULTS[lam][0]) < 1e-12
        # (b) clipped by hand, the ordered pass pays a jump into event 5
        clipped = dst.find_ordered_track(patterns, centres, cases.WINDOW, lam, order=True, reach=cases.CLIPPED)
        assert clipped.shifts == cases.TRUE_K and clipped.jumps == [5] and abs(clipped.cost - (found.cost + lam)) < 1e-12
        # (c) the ordered call refuses the unclipped reach
        with pytest.raises(SushiError) as e:
            dst.find_ordered_track(patterns, centres, cases.WINDOW, lam, order=True, max_rate=cases.MAX_RATE)
        assert "event 5" in str(e.value) and "2399" in str(e.value) and "1024" in str(e.value)
    # (d) margins, marginals, one chunk and 3 + 3 + 3 + 1 events; a penalty per event
    lam = cases.PENALTY
    want = track.track_ordered_margins_host(rows, w, lam, 0.0, cases.REACH, back, cases.GUARD, wide=True)
    for kw in (dict(), dict(max_bytes=4 * 3 * N + 3)):
        m = dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, [lam] * 10, order=True, max_rate=cases.MAX_RATE, margins=True,
                                        guard=cases.GUARD, marginals=True, **kw)
        _assert_track_equals(m, want, rows, K)
        assert (_bits64(m.event_through) == _bits64(want.through)).all()
        assert (_bits64(m.marginals.cpu().numpy()) == _bits64(want.marginals)).all()
        assert [None if k is None else k - K for k in m.event_alt_shift] == [None if k < 0 else k for k in want.alt_arg.tolist()]
        assert m.penalties == [0.0] + [lam] * 9 and m.guard == [cases.GUARD] * 10
    plain = dst.find_track(patterns, centres, cases.WINDOW, lam, max_rate=cases.MAX_RATE, wide=True, margins=True, guard=cases.GUARD)
    for v in cases.VICTIMS:
        assert abs(m.event_margin[v] - cases.ORDERED_MARGINS[v]) < 5e-4 and abs(plain.event_margin[v] - cases.PLAIN_MARGINS[v]) < 5e-4
        assert m.event_alt_shift[v] == cases.ORDERED_ALT_K[v]
    # order= as a list, and None (no limit, one penalty: the plain wide pass's result)
    listed = dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, lam, order=cases.BACK, max_rate=cases.MAX_RATE)
    assert listed.shifts == cases.TRUE_K and _bits64(listed.cost) == _bits64(want.cost)
    free = dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, lam, max_rate=cases.MAX_RATE)
    plain = dst.find_track(patterns, centres, cases.WINDOW, lam, max_rate=cases.MAX_RATE, wide=True)
    assert free.shifts == plain.shifts == cases.DECOYED_K and _bits64(free.cost) == _bits64(plain.cost) and free.jumps == plain.jumps
    # clamp=
    f = 0.6
    clamped = dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, lam, order=True, max_rate=cases.MAX_RATE, clamp=f)
    want_c = track.track_ordered_host([np.minimum(r, np.float32(f)) for r in rows], w, lam, 0.0, cases.REACH, back, wide=True)
    assert [k - K for k in clamped.shifts] == want_c.shifts.tolist() and _bits64(clamped.cost) == _bits64(want_c.cost)
    assert clamped.clamp is not None and clamped.rows_info is not None
    # its SushiErrors
    need = track.ordered_wide_state_bytes(10, N, margins=True)
    with pytest.raises(SushiError) as e:
        dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, lam, order=True, max_rate=cases.MAX_RATE, margins=True,
                                    max_state_bytes=need - 1)
    assert str(need) in str(e.value) and "window records" in str(e.value)
    with pytest.raises(SushiError) as e:
        dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, lam, order=True, max_rate=cases.MAX_RATE, step_cost=1e-3)
    assert "event 5" in str(e.value) and "2399" in str(e.value) and "0.001" in str(e.value)
    with pytest.raises(SushiError) as e:
        dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, lam, order=True, reach=[0] + [32768] * 9)
    assert "32768" in str(e.value) and "32767" in str(e.value)
    # shifts.calculate_ordered_wide_shifts passes everything through
    events = [ScriptEvent(s, e) for s, e in cases.EVENTS]
    got = calculate_ordered_wide_shifts(src, dst, events, cases.WINDOW, lam, max_rate=cases.MAX_RATE)
    assert got.shifts == cases.TRUE_K and _bits64(got.cost) == _bits64(want.cost)
    assert [ev.shift for ev in events] == got.deltas


def test_find_ordered_wide_track_in_float32_streams():
    """The same scenario in float32 streams, against the host restatement over the events' score curves on the joint axis."""
    from sushi_amd import axis
    from sushi_amd.curves import match_curves
    dst, src = cases.streams(sample_type='float32')
    patterns, centres, _bases = cases.scenario(dst, src)
    dst_dev = dst.device_stream()
    src_dev, offs, lens, _ = dst._pattern_source(patterns, dst_dev)
    lens = axis.pattern_lengths(lens)
    ax = axis.event_axis(dst, offs, lens, centres, cases.WINDOW)
    assert (ax.k_lo, ax.n_shift) == (cases.K_LO, cases.N_SHIFT)
    curves, at = match_curves(dst_dev, src_dev, ax.offs, lens, [b + ax.k_lo for b in ax.bases], [ax.n_shift] * 10)
    curves = curves.cpu().numpy()
    rows = [curves[at[k]:at[k + 1]] for k in range(10)]
    back = [ANY] + cases.BACK[1:]
    want = track.track_ordered_margins_host(rows, [1.0] * 10, cases.PENALTY, 0.0, cases.REACH, back, cases.GUARD, wide=True)
    found = dst.find_ordered_wide_track(patterns, centres, cases.WINDOW, cases.PENALTY, order=True, max_rate=cases.MAX_RATE, margins=True,
                                        guard=cases.GUARD)
    _assert_track_equals(found, want, rows, cases.K_LO)
    assert found.shifts == cases.TRUE_K and found.jumps == [] and found.reach == cases.REACH
    assert (_bits64(found.event_through) == _bits64(want.through)).all()
