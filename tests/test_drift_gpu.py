"""The drift search on the GPU: sushi_hip_drift_reduce against its NumPy restatement (sushi_amd/drift.py drift_host), bit for bit, on
the synthetic cases of tests/drift_cases.py; against sushi_hip_joint_reduce where the two coincide; WavStream.find_drift on a source
retimed by 2001/2000, against drift_host over the device's own rows and against the events' own minima; and
shifts.calculate_drifting_shifts."""
import numpy as np
import pytest

import drift_cases as cases
from sushi_amd import drift, joint
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, calculate_drifting_shifts

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_equals_host(res, want, case, with_lines):
    best, score, row_score, drift_idx, drift_score = (t.cpu().numpy() for t in res[:5])
    assert best.tolist() == [want.drift, want.index], (case.name, best.tolist(), want.drift, want.index)
    assert _bits(score)[0] == _bits(want.score), case.name
    assert (_bits(row_score) == _bits(want.row_scores)).all(), case.name
    assert (drift_idx == want.drift_index).all(), case.name
    assert (_bits(drift_score) == _bits(want.drift_scores)).all(), case.name
    if with_lines:
        assert res.lines.shape == want.lines.shape and (_bits(res.lines.cpu().numpy()) == _bits(want.lines)).all(), case.name
    else:
        assert res.lines is None
    if case.expect is not None:
        assert tuple(best.tolist()) == case.expect, case.name


# ---------------------------------------------------------------------------------------------- the reduce, synthetic rows
@pytest.fixture(scope="module", params=METHODS)
def synthetic(request):
    method = request.param
    all_cases = cases.grid_cases(method) + cases.special_cases(method)
    return method, all_cases, [drift.drift_host(*cases.rows_of(c), c.offsets, method) for c in all_cases]


def test_reduce_equals_drift_host(synthetic):
    """E of 1, 3, 4, 5, 9 x n_shift of 1, 63, 64, 65, 257, 513, 2049 with 1, DB - 1, DB, DB + 1 and 2 DB + 3 candidates of zero,
    negative, positive and mixed offsets; rows at odd offsets; weights 1/E, 1/3 and 0; a single-index range, a range that ends
    inside the last item, ties across a workgroup boundary and across candidates, signed zeros, all ones; with and without the
    lines."""
    import torch
    method, all_cases, want = synthetic
    for case, w in zip(all_cases, want):
        dev = torch.from_numpy(case.curves).cuda()
        _assert_equals_host(drift.drift_reduce_device(dev, case.rows, case.n_shift, case.offsets, method, with_lines=True), w, case, True)
        _assert_equals_host(drift.drift_reduce_device(dev, case.rows, case.n_shift, case.offsets, method), w, case, False)


def test_two_calls_on_two_streams(synthetic):
    import torch
    method, all_cases, want = synthetic
    by_name = {c.name: (c, w) for c, w in zip(all_cases, want)}
    (a_case, a_want), (b_case, b_want) = by_name["tie_across_workgroups_and_candidates"], by_name["range_ends_in_last_item"]
    a_dev, b_dev = torch.from_numpy(a_case.curves).cuda(), torch.from_numpy(b_case.curves).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = drift.drift_reduce_device(a_dev, a_case.rows, a_case.n_shift, a_case.offsets, method, with_lines=True, hip_stream=s1.cuda_stream)
    b = drift.drift_reduce_device(b_dev, b_case.rows, b_case.n_shift, b_case.offsets, method, with_lines=True, hip_stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _assert_equals_host(a, a_want, a_case, True)
    _assert_equals_host(b, b_want, b_case, True)


@pytest.mark.parametrize("method", METHODS)
def test_reduce_with_large_items(method):
    """2048 * 8 + 77 shifts (9 items of 2048) x 229 blocks of candidates: the size from which on a workgroup takes eight indices per thread; the last
    item is cut short, the last block holds one candidate, and the best lies in that candidate's last valid element."""
    import torch
    case = cases.large_case(method)
    want = drift.drift_host(*cases.rows_of(case), case.offsets, method)
    res = drift.drift_reduce_device(torch.from_numpy(case.curves).cuda(), case.rows, case.n_shift, case.offsets, method, with_lines=True)
    _assert_equals_host(res, want, case, True)


@pytest.mark.parametrize("method", METHODS)
def test_one_candidate_of_zeros_is_the_joint_reduce(method):
    import torch
    for case in cases.grid_cases(method)[10:] + cases.special_cases(method)[2:3]:
        dev = torch.from_numpy(case.curves).cuda()
        zeros = np.zeros((1, len(case.rows)), np.int32)
        a = drift.drift_reduce_device(dev, case.rows, case.n_shift, zeros, method, with_lines=True)
        b = joint.joint_reduce_device(dev, case.rows, [(0, len(case.rows), case.n_shift)], method, with_curve=True)
        assert a.best.cpu().tolist() == [0, int(b.index[0])], case.name
        assert (_bits(a.score.cpu().numpy()) == _bits(b.score.cpu().numpy())).all(), case.name
        assert (_bits(a.row_scores.cpu().numpy()) == _bits(b.row_scores.cpu().numpy())).all(), case.name
        assert (_bits(a.lines.cpu().numpy()[0]) == _bits(b.joint.cpu().numpy())).all(), case.name


def test_tables_are_checked_in_python():
    import torch
    dev = torch.zeros(100, dtype=torch.float32).cuda()
    for rows, n_shift, offsets in (([(0, 1.0)], 101, [[0]]), ([(-1, 1.0)], 10, [[0]]), ([(0, -1.0)], 10, [[0]]), ([(0, 1.0)], 0, [[0]]),
                                   ([], 10, np.zeros((1, 0), np.int32)), ([(0, 1.0)], 10, [[10]]), ([(0, 1.0), (50, 1.0)], 10, [[5, -5]]),
                                   ([(0, 1.0)], 10, np.zeros((0, 1), np.int32)), ([(0, 1.0)], 10, [[0, 0]])):
        with pytest.raises(SushiError):
            drift.drift_reduce_device(dev, rows, n_shift, offsets)
    with pytest.raises(SushiError):
        drift.drift_reduce_device(dev, [(0, 1.0)], 10, [[0]], method="sqdiff")
    with pytest.raises(SushiError):
        drift.drift_reduce_device(dev.cpu(), [(0, 1.0)], 10, [[0]])
    assert drift.drift_reduce_device(dev, [(0, 1.0), (50, 1.0)], 10, [[5, -4]]).best.cpu().tolist() == [0, 4]


# ---------------------------------------------------------------------------------------------- find_drift
@pytest.fixture(scope="module")
def retimed_case():
    dst, src = cases.drift_streams()
    patterns = [src.get_substream(s, s + cases.EVENT_LENGTH) for s in cases.EVENT_STARTS]
    found = dst.find_drift(patterns, cases.EVENT_STARTS, cases.WINDOW, cases.MAX_RATE, with_lines=True)
    return dst, src, patterns, found


def test_find_drift_finds_the_rate(retimed_case):
    _dst, _src, _patterns, found = retimed_case
    step = found.drift_rates[1] - found.drift_rates[0]
    print("rate %.9g (true %.9g, step %.3g), delta %.6f, score %.6g" % (found.rate, cases.TRUE_RATE, step, found.delta, found.score))
    assert found.drift_rates.shape == (661,) and found.drift_rates[330] == 0.0 and (found.k_lo, found.n_shift) == (-6000, 12001)
    assert abs(found.rate - cases.TRUE_RATE) <= step
    assert found.rate_ties[0] == found.rate == found.drift_rates[found.drift]      # the lowest of the rates that tie
    assert found.anchor == (2.0 + 57.0) / 2 and found.delta == (found.k_lo + found.index) / float(cases.RATE)
    # the profile over rate has its best at the answer and the shift at the anchor there
    assert int(np.argmin(found.drift_scores)) == found.drift and found.drift_deltas[found.drift] == found.delta
    assert _bits(found.drift_scores[found.drift]) == _bits(found.score)


def test_find_drift_equals_drift_host_over_the_device_rows(retimed_case):
    dst, _src, patterns, found = retimed_case
    rows = [r[0] for r in dst.match_templates(patterns, cases.EVENT_STARTS, [cases.WINDOW] * len(patterns))]
    bases = [dst._get_sample_for_time(s) for s in cases.EVENT_STARTS]
    offsets = drift.drift_offsets(bases, found.drift_rates)
    want = drift.drift_host(rows, [1.0 / len(rows)] * len(rows), offsets)
    assert (found.drift, found.index) == (want.drift, want.index) and _bits(found.score) == _bits(want.score)
    assert (_bits(found.event_scores) == _bits(want.row_scores)).all()
    assert (_bits(found.drift_scores) == _bits(want.drift_scores)).all()
    assert [round(d * cases.RATE) - found.k_lo for d in found.drift_deltas] == want.drift_index.tolist()
    assert (_bits(found.lines) == _bits(want.lines)).all()
    assert [round(d * cases.RATE) for d in found.event_deltas] == [found.k_lo + want.index + int(o) for o in offsets[want.drift]]
    own = joint.joint_host(rows, [1.0 / len(rows)] * len(rows))
    assert [round(d * cases.RATE) - found.k_lo for d in found.event_own_delta] == own.row_own_index.tolist()
    assert (_bits(found.event_own_scores) == _bits(own.row_own_scores)).all()


def test_every_event_lands_at_its_own_minimum(retimed_case):
    """Within EVENT_TOLERANCE = 2 samples of the event's own minimum in a +-16-sample neighbourhood of its true place t * 2001 /
    2000: <= 0.5 from half a grid step at the farthest event, <= 0.5 from rint, <= 1 from the two truncations (retimed's read
    positions, _get_sample_for_time).  tests/test_drift_host.py checks the same on the CPU oracle's rows (worst case there: 1)."""
    dst, _src, patterns, found = retimed_case
    worst = 0
    for e, (start, pattern) in enumerate(zip(cases.EVENT_STARTS, patterns)):
        base = dst._get_sample_for_time(start)
        on_line = base + round(found.event_deltas[e] * cases.RATE)
        centre = int(round(cases.true_place(dst, start)))
        first = centre - cases.NEIGHBOURHOOD
        worst = max(worst, abs(on_line - _own_minimum(dst, pattern, first, 2 * cases.NEIGHBOURHOOD + 1)))
    print("worst |event on the line - its own minimum| = %d samples" % worst)
    assert worst <= cases.EVENT_TOLERANCE


def _own_minimum(dst, pattern, first, count):
    """The first minimum of the pattern's exact scores at destination samples first .. first + count - 1."""
    from sushi_amd.curves import match_curves
    dst_dev = dst.device_stream()
    src_dev, offs, lens, _ = dst._pattern_source([pattern], dst_dev)
    curves, _bounds = match_curves(dst_dev, src_dev, offs, lens, [first], [count])
    return first + int(np.argmin(curves.cpu().numpy()))


def test_the_line_beats_the_constant_shift(retimed_case):
    dst, _src, patterns, found = retimed_case
    const = dst.find_joint(patterns, cases.EVENT_STARTS, cases.WINDOW)
    print("drift score %.6g, joint score %.6g; first event %.6g / %.6g, last %.6g / %.6g"
          % (found.score, const.score, found.event_scores[0], const.event_scores[0], found.event_scores[-1], const.event_scores[-1]))
    assert found.score < const.score
    assert found.event_scores[0] < const.event_scores[0] and found.event_scores[-1] < const.event_scores[-1]


def test_find_drift_refuses_what_it_cannot_do(retimed_case):
    dst, _src, patterns, found = retimed_case
    need = 4 * len(patterns) * found.n_shift
    with pytest.raises(SushiError) as e:
        dst.find_drift(patterns, cases.EVENT_STARTS, cases.WINDOW, cases.MAX_RATE, max_bytes=need - 1)
    assert str(need) in str(e.value)
    with pytest.raises(SushiError) as e:                      # +-0.01 s of window: 241 shifts; max_rate moves the ends 660 apart
        dst.find_drift(patterns, cases.EVENT_STARTS, 0.01, cases.MAX_RATE)
    assert "window_size" in str(e.value)
    with pytest.raises(SushiError) as e:
        dst.find_drift(patterns, cases.EVENT_STARTS, cases.WINDOW, 0.1)
    assert "D = " in str(e.value)
    with pytest.raises(SushiError):
        dst.find_drift(patterns, cases.EVENT_STARTS[:-1], cases.WINDOW, cases.MAX_RATE)
    with pytest.raises(SushiError):
        dst.find_drift(patterns, cases.EVENT_STARTS, cases.WINDOW, cases.MAX_RATE, method="sqdiff")


def test_calculate_drifting_shifts(retimed_case):
    dst, src, _patterns, found = retimed_case
    events = [ScriptEvent(s, s + cases.EVENT_LENGTH) for s in cases.EVENT_STARTS]
    match = calculate_drifting_shifts(src, dst, events, cases.WINDOW, cases.MAX_RATE)
    assert (match.drift, match.index) == (found.drift, found.index)
    for e, delta, score in zip(events, match.event_deltas, match.event_scores):
        assert e.shift == delta and _bits(e.diff) == _bits(score) and not e.linked
    assert len(set(e.shift for e in events)) > 6                # the shift moves along the programme
    # a centre shift moves the axis, not the answer: the events' shifts are the same instants
    events2 = [ScriptEvent(s, s + cases.EVENT_LENGTH) for s in cases.EVENT_STARTS]
    match2 = calculate_drifting_shifts(src, dst, events2, cases.WINDOW, cases.MAX_RATE, centre_shift=0.125)
    assert match2.rate == match.rate and match2.delta == match.delta - 0.125
    for a, b, delta in zip(events, events2, match2.event_deltas):
        assert b.shift == 0.125 + delta and abs(a.shift - b.shift) < 1e-9
    with pytest.raises(SushiError):
        calculate_drifting_shifts(src, dst, [ScriptEvent(5.0, 5.0)], cases.WINDOW, cases.MAX_RATE)
    with pytest.raises(SushiError):
        calculate_drifting_shifts(src, dst, [], cases.WINDOW, cases.MAX_RATE)
