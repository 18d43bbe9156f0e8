"""Tracking on the GPU: sushi_hip_track_forward / sushi_hip_track_backtrack against their NumPy restatement (sushi_amd/track.py
track_host), bit for bit down to the moves, on synthetic sequences; reach 0 against the segmentation pass; chunking; two streams;
WavStream.find_track against track_host over the CPU oracle's rows on the wandering-shift scenario of tests/test_track_host.py,
where find_segments fails as path_host does; shifts.calculate_tracked_shifts; a float32 case against match_templates rows."""
import numpy as np
import pytest

import track_cases as cases
from sushi_amd import segments, synth, track
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, calculate_tracked_shifts
from sushi_amd.wav import WavStream

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")
RATE = 12000
JUMP = -32768


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(curves_dev, rows, reach, n, lam, mu, method, chunks=None, hip_stream=None):
    """The whole pass on the device: forward calls over `chunks` (row counts; default: one call), then the backtrack."""
    state = track.TrackState(len(rows), n, curves_dev.device)
    row0 = 0
    for count in chunks or [len(rows)]:
        track.track_device(curves_dev, rows[row0:row0 + count], reach[row0:row0 + count], lam, mu, state, row0=row0, method=method,
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


# ---------------------------------------------------------------------------------------------- the pass, synthetic rows
@pytest.fixture(scope="module", params=METHODS)
def sequences(request):
    """One sequence per shape of cases.SHAPES, with track_host's answer: computed once."""
    out = {}
    for E, n, reach in cases.SHAPES:
        curves, rows, weights, lam, rs, mu = cases.sequence(E, n, reach, request.param, seed=3)
        out[(E, n, reach)] = (curves, rows, rs, lam, mu, track.track_host(cases.rows_of(curves, rows, n), weights, lam, mu, rs, request.param))
    return request.param, out


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_pass_equals_track_host(sequences, shape):
    """(rows, shifts, reach) = (1, 1, 0) (2, 63, 1) (7, 64, 3) (9, 65, 64) (33, 1023, 127) (3, 4097, 1024) (16, 70001, 5): wave,
    workgroup and work-item edges; every halo size (none, two rounds, eight rounds), a reach wider than a work item of 512 and wider
    than the axis; rows at odd offsets in shuffled order; a reach that varies by row; weights 1, 1/3, 0 and 2.5; equal minima across a
    workgroup boundary (511 | 512) and in the last element, an all-ones sequence.  Shifts, cost, row_min, row_arg, own index, own
    score and every move: bitwise."""
    import torch
    method, table = sequences
    curves, rows, rs, lam, mu, want = table[shape]
    assert all(o % 2 == 1 for o, _w in rows) and (len(rs) < 3 or len(set(rs[1:])) > 1 or shape[2] == 0)
    if shape == (9, 65, 64):
        assert want.shifts.tolist() == [0] * 9 and not want.moves.any()
    if shape[1] >= 8 and shape != (9, 65, 64):
        words = [int(want.moves[e, want.shifts[e]]) for e in range(1, shape[0])]
        assert any(w not in (0, JUMP) for w in words) and (JUMP in words) == (shape[0] >= 7)       # paths that do move, and jump
    state, shifts = _run(torch.from_numpy(curves).cuda(), rows, rs, shape[1], lam, mu, method)
    _assert_equals_host(state, shifts, want)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("centre", [511, 512])
def test_ties_whose_sides_lie_in_different_work_items(centre, method):
    """1024 shifts are two work items of 512.  cand(-1) == cand(+1) at `centre`, one side in each item: -1 wins; cand(0) ==
    cand(+-1) at shifts 0 and 1023 with free moves: 0 wins."""
    import torch
    a, b = cases.tie_rows(1024, centre, method)
    curves = np.concatenate([np.zeros(1, np.float32), a, np.zeros(2, np.float32), b])
    rows = [(1, 1.0), (1027, 1.0)]
    want = track.track_host([a, b], [1.0, 1.0], 0.5, 0.0, [0, 3], method)
    assert want.moves[1, centre] == -1 and want.moves[1, 0] == 0 and want.moves[1, 1023] == 0
    assert want.moves[1, centre - 2] == 1 and want.moves[1, centre + 2] == -1
    state, shifts = _run(torch.from_numpy(curves).cuda(), rows, [0, 3], 1024, 0.5, 0.0, method)
    _assert_equals_host(state, shifts, want)


@pytest.mark.parametrize("method", METHODS)
def test_the_tie_between_moving_and_jumping_and_a_reach_beyond_the_axis(method):
    import torch
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    up = np.nextafter(np.float32(0.5), np.float32(1.0))
    curves = np.array([0.25, 0.5, 1.0, 0.75, 0.75, -0.25, 0.25, up, 1.0], np.float32) * sign
    dev = torch.from_numpy(curves).cuda()
    # D_0 = [0.25, 0.5, 1.0], mu = 0.25, lam = 0.5: at j = 2, near = 0.5 + 0.25 = jump: the tie moves; one ulp above it jumps
    for first, word, path in ((0, -1, [1, 2]), (6, JUMP, [0, 2])):
        rows = [(first, 1.0), (3, 1.0)]
        want = track.track_host(cases.rows_of(curves, rows, 3), [1.0, 1.0], 0.5, 0.25, [0, 1], method)
        assert want.moves[1, 2] == word and want.shifts.tolist() == path and want.cost == 0.5
        _assert_equals_host(*_run(dev, rows, [0, 1], 3, 0.5, 0.25, method), want)
    # n_shift < reach: 5 and 7 shifts under reaches up to 1024
    for E, n, reach in ((3, 5, 1024), (4, 7, 64)):
        curves, rows, weights, lam, rs, mu = cases.sequence(E, n, reach, method, seed=5)
        want = track.track_host(cases.rows_of(curves, rows, n), weights, lam, mu, rs, method)
        _assert_equals_host(*_run(torch.from_numpy(curves).cuda(), rows, rs, n, lam, mu, method), want)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [cases.PER_LARGE_FROM, cases.PER_LARGE_FROM - 1])
def test_pass_at_the_size_where_the_split_changes(n, method):
    """The shifts from which on a workgroup takes eight indices per thread (1024 items of 2048), and one shift below it (4092 items
    of 512: a grid of 2048 strides over them, and stages a tile per item).  Two rows, reach 2; the minimum lies twice in the last,
    cut item's last elements."""
    import torch
    E = 2
    rng = np.random.default_rng(19)
    lo = 0.25 if method == "sqdiff_normed" else -0.5
    curves = rng.random(E * (n + 3) + 8, dtype=np.float32) * np.float32(0.5) + np.float32(lo)
    rows = [(1 + e * (n + 3) + 2 * (e % 2), (1.0, 1.0 / 3.0)[e]) for e in range(E)]
    best = np.float32(0.125 if method == "sqdiff_normed" else 0.875)
    for o, _w in rows:
        curves[o + n - 2] = curves[o + n - 1] = best
    want = track.track_host(cases.rows_of(curves, rows, n), [w for _o, w in rows], 1.0, cases.STEP_COST, [0, 2], method)
    assert want.shifts.tolist() == [n - 2] * E and np.count_nonzero(want.moves[1] > 0) > n // 8
    _assert_equals_host(*_run(torch.from_numpy(curves).cuda(), rows, [0, 2], n, 1.0, cases.STEP_COST, method), want)


def test_a_sequence_in_chunks_has_the_bits_of_one_call(sequences):
    import torch
    method, table = sequences
    curves, rows, rs, lam, mu, want = table[(33, 1023, 127)]
    dev = torch.from_numpy(curves).cuda()
    whole, shifts = _run(dev, rows, rs, 1023, lam, mu, method)
    _assert_equals_host(whole, shifts, want)
    for chunks in ([1, 15, 17], [2, 31]):            # a later call's row0 odd and even
        parts, shifts_parts = _run(dev, rows, rs, 1023, lam, mu, method, chunks=chunks)
        assert torch.equal(shifts, shifts_parts)
        for a, b in zip(whole.tensors()[1:], parts.tensors()[1:]):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        assert torch.equal(whole.last_D().view(torch.int64), parts.last_D().view(torch.int64))
    with pytest.raises(SushiError):
        track.track_device(dev, rows[:2], rs[:2], lam, mu, parts, row0=32, method=method)       # rows 32 .. 33 of 33
    with pytest.raises(SushiError):
        track.track_device(dev, [(len(curves) - 1022, 1.0)], [0], lam, mu, parts, method=method)
    with pytest.raises(SushiError):
        track.track_device(dev, rows[1:3], [1025, 1], lam, mu, parts, row0=1, method=method)


def test_two_sequences_on_two_streams(sequences):
    import torch
    method, table = sequences
    curves_a, rows_a, rs_a, lam_a, mu_a, want_a = table[(16, 70001, 5)]
    curves_b, rows_b, rs_b, lam_b, mu_b, want_b = table[(33, 1023, 127)]
    dev_a, dev_b = torch.from_numpy(curves_a).cuda(), torch.from_numpy(curves_b).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, shifts_a = _run(dev_a, rows_a, rs_a, 70001, lam_a, mu_a, method, hip_stream=s1.cuda_stream)
    b, shifts_b = _run(dev_b, rows_b, rs_b, 1023, lam_b, mu_b, method, chunks=[16, 17], hip_stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _assert_equals_host(a, shifts_a, want_a)
    _assert_equals_host(b, shifts_b, want_b)


def test_all_reach_zero_is_the_segmentation_pass(sequences):
    import torch
    method, table = sequences
    for shape in ((33, 1023, 127), (16, 70001, 5)):
        curves, rows, _rs, lam, _mu, _want = table[shape]
        dev = torch.from_numpy(curves).cuda()
        n = shape[1]
        got, shifts = _run(dev, rows, [0] * len(rows), n, lam, 0.5, method)
        ref = segments.PathState(len(rows), n, dev.device)
        segments.path_device(dev, rows, lam, ref, method=method)
        assert torch.equal(shifts, segments.path_backtrack_device(ref))
        for name in ("row_min", "row_arg", "row_own_index", "row_own_scores"):
            assert torch.equal(getattr(got, name).view(torch.uint8), getattr(ref, name).view(torch.uint8)), name
        assert torch.equal(got.last_D().view(torch.int64), ref.D.view(torch.int64))
        assert set(np.unique(got.moves.cpu().numpy()).tolist()) <= {0, JUMP}


# ---------------------------------------------------------------------------------------------- find_track
@pytest.fixture(scope="module")
def wander(oracle):
    dst, src = cases.streams()
    patterns, centres, bases = cases.scenario(dst, src)
    found = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, max_rate=cases.MAX_RATE)
    rows = cases.oracle_rows(oracle, dst, patterns, bases, cases.K_LO, cases.N_SHIFT)
    return dst, src, patterns, centres, bases, found, rows


def _assert_track_equals(found, want, rows, k_lo, rate):
    assert [k - k_lo for k in found.shifts] == want.shifts.tolist() and _bits64(found.cost) == _bits64(want.cost)
    assert found.deltas == [k / float(rate) for k in found.shifts]
    assert (_bits(found.event_scores) == _bits([r[s] for r, s in zip(rows, want.shifts)])).all()
    assert [round(d * rate) - k_lo for d in found.event_own_delta] == want.row_own_index.tolist()
    assert (_bits(found.event_own_scores) == _bits(want.row_own_scores)).all()
    E = len(rows)
    jumps = [e for e in range(1, E) if want.moves[e, want.shifts[e]] == JUMP]
    assert found.jumps == jumps and found.moves == [0] + np.diff(want.shifts).tolist()
    assert found.segments == [(f, n, found.deltas[f], found.deltas[f + n - 1]) for f, n in track.jump_runs(E, jumps)]
    assert sum(n for _f, n, _a, _b in found.segments) == E


def test_the_wandering_shift_scenario_on_the_gpu(wander):
    """tests/test_track_host.py's scenario and its recorded oracle results: lone searches return the decoys, find_segments fails at
    every penalty as path_host does, find_track returns the ten true shifts -- with the oracle's bits."""
    dst, _src, patterns, centres, _bases, found, rows = wander
    _scores, _times, index = dst.find_substreams(patterns, centres, [cases.WINDOW] * 10, with_index=True)
    assert [i - dst._get_sample_for_time(c) for i, c in zip(index, centres)] == cases.LONE_K
    for lam, shifts, cost in cases.PATH_RESULTS:
        seg = dst.find_segments(patterns, centres, cases.WINDOW, lam)
        assert seg.shifts == shifts != cases.TRUE_K and seg.cost == cost, lam
    assert (found.k_lo, found.n_shift, found.reach) == (cases.K_LO, cases.N_SHIFT, cases.REACH)
    assert found.shifts == cases.TRUE_K and found.cost == cases.TRACK_COSTS[(cases.PENALTY, 0.0)]
    assert found.jumps == cases.JUMPS
    assert found.segments == [(0, 5, 3000 / 12000.0, 2990 / 12000.0), (5, 5, -2400 / 12000.0, -2300 / 12000.0)]
    assert _bits(found.event_scores).tolist() == cases.EVENT_SCORE_BITS
    assert [round(d * cases.RATE) for d in found.event_own_delta] == cases.LONE_K
    assert _bits(found.event_own_scores).tolist() == cases.OWN_SCORE_BITS
    _assert_track_equals(found, track.track_host(rows, [1.0] * 10, cases.PENALTY, 0.0, cases.REACH), rows, cases.K_LO, cases.RATE)


def test_every_penalty_and_step_cost_of_the_scenario(wander):
    dst, _src, patterns, centres, _bases, _found, rows = wander
    for (lam, mu), cost in sorted(cases.TRACK_COSTS.items()):
        if (lam, mu) == (cases.PENALTY, 0.0):
            continue
        got = dst.find_track(patterns, centres, cases.WINDOW, lam, reach=cases.REACH, step_cost=mu)
        assert got.shifts == cases.TRUE_K and got.cost == cost, (lam, mu)
    far = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY_TOO_LARGE, max_rate=cases.MAX_RATE)
    assert far.shifts == cases.TOO_LARGE_K and far.jumps == []
    _assert_track_equals(far, track.track_host(rows, [1.0] * 10, cases.PENALTY_TOO_LARGE, 0.0, cases.REACH), rows, cases.K_LO, cases.RATE)


def test_three_chunks_weights_and_method(oracle, wander):
    dst, _src, patterns, centres, bases, found, rows = wander
    chunked = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, max_rate=cases.MAX_RATE,
                             max_bytes=4 * 3 * cases.N_SHIFT + 3)                      # 3 + 3 + 3 + 1 events: row0 odd and even
    assert (chunked.shifts, chunked.deltas, chunked.segments, chunked.jumps, chunked.moves, chunked.event_own_delta) == \
        (found.shifts, found.deltas, found.segments, found.jumps, found.moves, found.event_own_delta)
    assert _bits64(chunked.cost) == _bits64(found.cost)
    for name in ("event_scores", "event_own_scores"):
        assert (_bits(getattr(chunked, name)) == _bits(getattr(found, name))).all(), name
    lens = [p.shape[1] for p in patterns]
    by_length = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, reach=cases.REACH, step_cost=1e-3, weights="length")
    explicit = [float(m) * 10 / float(sum(lens)) for m in lens]
    _assert_track_equals(by_length, track.track_host(rows, explicit, cases.PENALTY, 1e-3, cases.REACH), rows, cases.K_LO, cases.RATE)
    cc_rows = cases.oracle_rows(oracle, dst, patterns, bases, cases.K_LO, cases.N_SHIFT, method="ccoeff_normed")
    got = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, max_rate=cases.MAX_RATE, method="ccoeff_normed")
    _assert_track_equals(got, track.track_host(cc_rows, [1.0] * 10, cases.PENALTY, 0.0, cases.REACH, "ccoeff_normed"), cc_rows,
                         cases.K_LO, cases.RATE)
    # all reach 0: find_segments' answer
    rigid = dst.find_track(patterns, centres, cases.WINDOW, 0.25, reach=0)
    seg = dst.find_segments(patterns, centres, cases.WINDOW, 0.25)
    assert rigid.shifts == seg.shifts and _bits64(rigid.cost) == _bits64(seg.cost)
    need = track.TrackState.nbytes(10, cases.N_SHIFT)
    with pytest.raises(SushiError) as e:
        dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, max_rate=cases.MAX_RATE, max_state_bytes=need - 1)
    assert str(need) in str(e.value)
    with pytest.raises(SushiError) as e:
        dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, max_rate=0.1)
    assert "event 1" in str(e.value) and "1441" in str(e.value)
    for bad in (dict(), dict(max_rate=1e-3, reach=1), dict(reach=1, step_cost=-1.0), dict(reach=1, method="sqdiff")):
        with pytest.raises(SushiError):
            dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, **bad)


def test_find_track_f32_equals_track_host_over_match_templates():
    dst_pcm = synth.make_dst_pcm(12, RATE, seed=31)
    src_pcm = synth.make_src_pcm(dst_pcm, [(0, 1500), (37000, 1530), (60000, -900), (82000, -925)], seed=32)
    dst, src = (WavStream.from_samples(p, RATE, sample_type='float32') for p in (dst_pcm, src_pcm))
    spans = [(2.0, 2.5), (3.25, 3.75), (6.0, 6.625), (7.5, 7.875)]
    patterns, centres = [src.get_substream(s, e) for s, e in spans], [s for s, _e in spans]
    rows = [r[0] for r in dst.match_templates(patterns, centres, [0.5] * 4)]
    reach = track.rate_reach([dst._get_sample_for_time(c) for c in centres], 3e-3)
    assert reach == [0, 46, 100, 55]
    want = track.track_host(rows, [1.0] * 4, 0.25, 1e-4, reach)
    got = dst.find_track(patterns, centres, 0.5, 0.25, max_rate=3e-3, step_cost=1e-4)
    assert (got.k_lo, got.n_shift) == (-6000, 12001) and got.n_shift == rows[0].shape[0]
    _assert_track_equals(got, want, rows, got.k_lo, RATE)
    assert got.shifts == [1500, 1530, -900, -925] and got.jumps == [2]


def test_calculate_tracked_shifts(wander):
    dst, src, _patterns, _centres, _bases, found, _rows = wander
    events = [ScriptEvent(s, e) for s, e in cases.EVENTS]
    got = calculate_tracked_shifts(src, dst, events, cases.WINDOW, cases.PENALTY, max_rate=cases.MAX_RATE)
    assert got.shifts == found.shifts and got.segments == found.segments and got.jumps == found.jumps
    for e, k, score in zip(events, cases.TRUE_K, found.event_scores):
        assert e.shift == k / float(cases.RATE) and _bits(e.diff) == _bits(score) and not e.linked
    # a centre shift a quarter of a second off: the deltas move by it, the events land where they did
    moved = calculate_tracked_shifts(src, dst, events, cases.WINDOW, cases.PENALTY, reach=cases.REACH, centre_shift=0.25)
    assert [k + 3000 for k in moved.shifts] == found.shifts and _bits64(moved.cost) == _bits64(found.cost)
    # (0.25 + a delta rounds: the events' shifts are compared in samples)
    assert [int(round(e.shift * cases.RATE)) for e in events] == found.shifts
    assert all(abs(e.shift - d) < 1e-12 for e, d in zip(events, found.deltas))
    with pytest.raises(SushiError):
        calculate_tracked_shifts(src, dst, [ScriptEvent(5.0, 5.0)], cases.WINDOW, cases.PENALTY, reach=1)
    with pytest.raises(SushiError):
        calculate_tracked_shifts(src, dst, [], cases.WINDOW, cases.PENALTY, reach=1)
