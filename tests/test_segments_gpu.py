"""Segmentation on the GPU: sushi_hip_path_forward / sushi_hip_path_backtrack against their NumPy restatement (sushi_amd/segments.py
path_host), bit for bit, on synthetic sequences; WavStream.find_segments against path_host over the CPU oracle's rows and against
lone searches; chunking, a stream end, the two-cut scenario of tests/test_segments_host.py, and shifts.calculate_segmented_shifts."""
import numpy as np
import pytest

import segment_cases as cases
from sushi_amd import joint, segments, synth
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, calculate_segmented_shifts
from sushi_amd.wav import WavStream

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")
RATE = 12000


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _run(curves_dev, rows, n, lam, method, chunks=None, hip_stream=None):
    """The whole pass on the device: forward calls over `chunks` (row counts; default: one call), then the backtrack."""
    state = segments.PathState(len(rows), n, curves_dev.device)
    row0 = 0
    for count in chunks or [len(rows)]:
        segments.path_device(curves_dev, rows[row0:row0 + count], lam, state, row0=row0, method=method, hip_stream=hip_stream)
        row0 += count
    assert row0 == len(rows)
    return state, segments.path_backtrack_device(state, hip_stream=hip_stream)


def _assert_equals_host(state, shifts, want, stay=None):
    assert shifts.cpu().numpy().tolist() == want.shifts.tolist()
    row_min = state.row_min.cpu().numpy()
    assert (_bits64(row_min) == _bits64(want.row_min)).all() and _bits64(row_min[-1]) == _bits64(want.cost)
    assert state.row_arg.cpu().numpy().tolist() == want.row_arg.tolist()
    assert state.row_own_index.cpu().numpy().tolist() == want.row_own_index.tolist()
    assert (_bits(state.row_own_scores.cpu().numpy()) == _bits(want.row_own_scores)).all()
    if stay is not None:
        assert (state.stay.cpu().numpy().view(np.uint64) == stay.reshape(-1)).all()


# ---------------------------------------------------------------------------------------------- the pass, synthetic rows
@pytest.fixture(scope="module", params=METHODS)
def sequences(request):
    """One sequence per shape of cases.SHAPES, with path_host's answer and the stay bits of the definition: computed once."""
    out = {}
    for E, n in cases.SHAPES:
        curves, rows, weights, lam = cases.sequence(E, n, request.param, seed=3)
        host_rows = cases.rows_of(curves, rows, n)
        out[(E, n)] = (curves, rows, lam, segments.path_host(host_rows, weights, lam, request.param),
                       cases.stay_words(host_rows, weights, lam, request.param))
    return request.param, out


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_pass_equals_path_host(sequences, shape):
    """(rows, shifts) = (1, 1) (2, 63) (7, 64) (9, 65) (33, 1023) (3, 4097) (16, 70001): wave, workgroup and work-item edges; rows at
    odd offsets in shuffled order; weights 1, 1/3, 0 and 2.5; a minimum tie across a workgroup boundary (511 | 512), one in the last
    element, an all-ones sequence.  Shifts, cost, row_min, row_arg, own index, own score and every stay word: bitwise."""
    import torch
    method, table = sequences
    curves, rows, lam, want, stay = table[shape]
    assert all(o % 2 == 1 for o, _w in rows)
    planted = {(33, 1023): [511] * 33, (3, 4097): [4095] * 3, (9, 65): [0] * 9}
    if shape in planted:
        assert want.shifts.tolist() == planted[shape]
    if shape in ((7, 64), (16, 70001)):
        assert len(segments.runs(want.shifts.tolist())) > 1                 # paths that do change
    state, shifts = _run(torch.from_numpy(curves).cuda(), rows, shape[1], lam, method)
    _assert_equals_host(state, shifts, want, stay)


@pytest.mark.parametrize("method", METHODS)
def test_the_exact_tie_between_staying_and_jumping(method):
    import torch
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    curves = np.array([0.75, 0.25, 0.25, 0.75, 9, 0.25, 0.75, 0.25, 0.75], np.float32) * sign
    dev = torch.from_numpy(curves).cuda()
    # D_0 = [0.75, 0.25], jump_1 = 0.25 + 0.5 = D_0[0]: index 0 stays, D_1 = [1, 1], the first index wins
    for rows, shifts, cost in (([(0, 1.0), (2, 1.0)], [0, 0], 1.0), ([(5, 1.0), (7, 1.0)], [0, 0], 0.5)):
        want = segments.path_host(cases.rows_of(curves, rows, 2), [1.0, 1.0], 0.5, method)
        state, got = _run(dev, rows, 2, 0.5, method)
        _assert_equals_host(state, got, want, cases.stay_words(cases.rows_of(curves, rows, 2), [1.0, 1.0], 0.5, method))
        if method == "sqdiff_normed":
            assert want.shifts.tolist() == shifts and want.cost == cost
    assert state.stay.cpu().numpy().tolist() == [0, 3]                      # row 0 has no bits; row 1: both indices stay


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("E,n", [(3, cases.PER_LARGE_FROM), (2, cases.PER_LARGE_FROM - 1), (2, 2048 * 2048 + 2049)])
def test_pass_at_the_sizes_where_the_split_changes(E, n, method):
    """The shifts from which on a workgroup takes eight indices per thread (1024 items of 2048); one shift below it (4092 items of
    512: a grid of 2048 strides over them); and 2049 items of 2048 (the same with eight per thread).  The minimum lies twice in the
    last, cut item's last elements."""
    import torch
    rng = np.random.default_rng(17 + E)
    lo = 0.25 if method == "sqdiff_normed" else -0.5
    curves = rng.random(E * (n + 3) + 8, dtype=np.float32) * np.float32(0.5) + np.float32(lo)
    rows = [(1 + e * (n + 3) + 2 * (e % 2), (1.0, 1.0 / 3.0, 2.5)[e]) for e in range(E)]
    best = np.float32(0.125 if method == "sqdiff_normed" else 0.875)
    for o, _w in rows:
        curves[o + n - 2] = curves[o + n - 1] = best
    curves[rows[0][0] + 2047] = curves[rows[0][0] + 2048] = np.float32(0.1875 if method == "sqdiff_normed" else 0.125)
    host_rows, weights = cases.rows_of(curves, rows, n), [w for _o, w in rows]
    want = segments.path_host(host_rows, weights, 0.0625, method)
    assert want.shifts.tolist() == [n - 2] * E
    state, shifts = _run(torch.from_numpy(curves).cuda(), rows, n, 0.0625, method)
    _assert_equals_host(state, shifts, want, cases.stay_words(host_rows, weights, 0.0625, method))


def test_a_sequence_in_chunks_has_the_bits_of_one_call(sequences):
    import torch
    method, table = sequences
    curves, rows, lam, want, stay = table[(33, 1023)]
    dev = torch.from_numpy(curves).cuda()
    whole, shifts = _run(dev, rows, 1023, lam, method)
    parts, shifts_parts = _run(dev, rows, 1023, lam, method, chunks=[1, 15, 17])
    _assert_equals_host(parts, shifts_parts, want, stay)
    assert torch.equal(shifts, shifts_parts)
    for a, b in zip(whole.tensors(), parts.tensors()):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    with pytest.raises(SushiError):
        segments.path_device(dev, rows[:2], lam, parts, row0=32, method=method)       # rows 32 .. 33 of 33
    with pytest.raises(SushiError):
        segments.path_device(dev, [(len(curves) - 1022, 1.0)], lam, parts, method=method)


def test_two_sequences_on_two_streams(sequences):
    import torch
    method, table = sequences
    curves_a, rows_a, lam_a, want_a, stay_a = table[(16, 70001)]
    curves_b, rows_b, lam_b, want_b, stay_b = table[(33, 1023)]
    dev_a, dev_b = torch.from_numpy(curves_a).cuda(), torch.from_numpy(curves_b).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a, shifts_a = _run(dev_a, rows_a, 70001, lam_a, method, hip_stream=s1.cuda_stream)
    b, shifts_b = _run(dev_b, rows_b, 1023, lam_b, method, chunks=[16, 17], hip_stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _assert_equals_host(a, shifts_a, want_a, stay_a)
    _assert_equals_host(b, shifts_b, want_b, stay_b)


# ---------------------------------------------------------------------------------------------- find_segments
@pytest.fixture(scope="module")
def two_cut(oracle):
    dst, src = cases.two_cut_streams()
    patterns, centres, bases = cases.scenario(dst, src)
    found = dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY)
    rows = cases.oracle_rows(oracle, dst, patterns, bases, cases.K_LO, cases.N_SHIFT)
    return dst, src, patterns, centres, bases, found, rows


def _assert_segmentation_equals(found, want, rows, k_lo, rate):
    assert [k - k_lo for k in found.shifts] == want.shifts.tolist() and _bits64(found.cost) == _bits64(want.cost)
    assert found.deltas == [k / float(rate) for k in found.shifts]
    assert (_bits(found.event_scores) == _bits([r[s] for r, s in zip(rows, want.shifts)])).all()
    assert [round(d * rate) - k_lo for d in found.event_own_delta] == want.row_own_index.tolist()
    assert (_bits(found.event_own_scores) == _bits(want.row_own_scores)).all()
    assert found.segments == [(f, n, (k_lo + s) / float(rate)) for f, n, s in segments.runs(want.shifts.tolist())]


def test_the_two_cut_scenario_on_the_gpu(two_cut):
    """tests/test_segments_host.py's scenario and its recorded oracle results: lone searches return the decoys, one joint search
    over all ten events returns the second half's shift, find_segments the two segments -- with the oracle's bits."""
    dst, _src, patterns, centres, _bases, found, rows = two_cut
    _scores, _times, index = dst.find_substreams(patterns, centres, [cases.WINDOW] * 10, with_index=True)
    assert [i - dst._get_sample_for_time(c) for i, c in zip(index, centres)] == cases.LONE_K
    assert dst.find_joint(patterns, centres, cases.WINDOW).delta == cases.JOINT_K / float(cases.RATE)
    assert (found.k_lo, found.n_shift) == (cases.K_LO, cases.N_SHIFT)
    assert found.shifts == cases.TRUE_K and found.cost == cases.COST
    assert found.segments == [(0, 5, 3000 / 12000.0), (5, 5, -2400 / 12000.0)]
    assert _bits(found.event_scores).tolist() == cases.EVENT_SCORE_BITS
    assert [round(d * cases.RATE) for d in found.event_own_delta] == cases.LONE_K
    assert _bits(found.event_own_scores).tolist() == cases.OWN_SCORE_BITS
    _assert_segmentation_equals(found, segments.path_host(rows, [1.0] * 10, cases.PENALTY), rows, cases.K_LO, cases.RATE)


def test_three_chunks_give_the_same_bits(two_cut):
    dst, _src, patterns, centres, _bases, found, rows = two_cut
    chunked = dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY, max_bytes=4 * 4 * cases.N_SHIFT + 3)   # 4 + 4 + 2 events
    assert (chunked.shifts, chunked.deltas, chunked.segments, chunked.event_own_delta) == \
        (found.shifts, found.deltas, found.segments, found.event_own_delta)
    assert _bits64(chunked.cost) == _bits64(found.cost)
    for name in ("event_scores", "event_own_scores"):
        assert (_bits(getattr(chunked, name)) == _bits(getattr(found, name))).all(), name
    with pytest.raises(SushiError) as e:
        dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY, max_bytes=4 * cases.N_SHIFT - 1)
    assert str(4 * cases.N_SHIFT) in str(e.value)
    need = segments.PathState.nbytes(10, cases.N_SHIFT)
    with pytest.raises(SushiError) as e:
        dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY, max_state_bytes=need - 1)
    assert str(need) in str(e.value)


def test_event_own_results_are_the_lone_searches(two_cut):
    dst, _src, patterns, centres, bases, found, _rows = two_cut
    scores, _times, index = dst.find_substreams(patterns, centres, [cases.WINDOW] * 10, with_index=True)
    assert [b + round(d * cases.RATE) for b, d in zip(bases, found.event_own_delta)] == index
    assert (_bits(found.event_own_scores) == _bits(scores)).all()


def test_weights_method_and_penalty(oracle, two_cut):
    dst, _src, patterns, centres, _bases, found, rows = two_cut
    lens = [p.shape[1] for p in patterns]
    by_length = dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY, weights="length")
    explicit = [float(m) * 10 / float(sum(lens)) for m in lens]
    _assert_segmentation_equals(by_length, segments.path_host(rows, explicit, cases.PENALTY), rows, cases.K_LO, cases.RATE)
    assert _bits64(by_length.cost) != _bits64(found.cost)
    free = dst.find_segments(patterns, centres, cases.WINDOW, 0.0, weights=[1.0] * 10)
    assert free.shifts == cases.LONE_K and free.cost == cases.EXTREMES[0][2]
    cc_rows = cases.oracle_rows(oracle, dst, patterns, _bases, cases.K_LO, cases.N_SHIFT, method="ccoeff_normed")
    got = dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY, method="ccoeff_normed")
    _assert_segmentation_equals(got, segments.path_host(cc_rows, [1.0] * 10, cases.PENALTY, "ccoeff_normed"), cc_rows, cases.K_LO,
                                cases.RATE)
    for bad in (dict(weights="median"), dict(weights=[1.0]), dict(method="sqdiff")):
        with pytest.raises(SushiError):
            dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY, **bad)
    for lam in (-0.5, float("nan"), float("inf")):
        with pytest.raises(SushiError):
            dst.find_segments(patterns, centres, cases.WINDOW, lam)


def test_find_segments_f32_equals_path_host_over_match_templates():
    dst_pcm = synth.make_dst_pcm(12, RATE, seed=31)
    src_pcm = synth.make_src_pcm(dst_pcm, [(0, 1500), (60000, -900)], seed=32)
    dst, src = (WavStream.from_samples(p, RATE, sample_type='float32') for p in (dst_pcm, src_pcm))
    spans = [(2.0, 2.5), (3.25, 3.75), (6.0, 6.625), (7.5, 7.875)]
    patterns, centres = [src.get_substream(s, e) for s, e in spans], [s for s, _e in spans]
    rows = [r[0] for r in dst.match_templates(patterns, centres, [0.5] * 4)]
    want = segments.path_host(rows, [1.0] * 4, 0.25)
    got = dst.find_segments(patterns, centres, 0.5, 0.25)
    assert (got.k_lo, got.n_shift) == (-6000, 12001) and got.n_shift == rows[0].shape[0]
    _assert_segmentation_equals(got, want, rows, got.k_lo, RATE)
    assert got.shifts == [1500, 1500, -900, -900]


def test_an_event_at_a_stream_end_cuts_the_axis(oracle, two_cut):
    dst, src = two_cut[0], two_cut[1]
    pad, total = dst.padding_size, dst.data.shape[1]
    patterns = [src.get_substream(1.0, 1.5), src.get_substream(9.4, 10.1), src.get_substream(13.0, 13.5)]
    last = (total - pad - 6000 - 3000) / float(RATE)     # a quarter of a second in front of the last fitting place
    centres = [-9.5, 9.4, last]                           # half a second into the left padding
    bases = [dst._get_sample_for_time(c) for c in centres]
    assert bases[0] == pad - int(9.5 * RATE) and bases[2] == total - 6000 - 3000
    got = dst.find_segments(patterns, centres, 1.0, 0.25)
    assert (got.k_lo, got.n_shift) == (-6000, 9001)
    rows = cases.oracle_rows(oracle, dst, patterns, bases, got.k_lo, got.n_shift)
    _assert_segmentation_equals(got, segments.path_host(rows, [1.0] * 3, 0.25), rows, got.k_lo, RATE)
    with pytest.raises(SushiError):
        dst.find_segments(patterns, [-10.5, 9.4, last + 0.25], 1.0, 0.25)      # the first event needs k >= 6000, the last k <= 0
    with pytest.raises(SushiError):
        dst.find_segments([patterns[0], patterns[1][:, :0]], centres[:2], 1.0, 0.25)


def test_calculate_segmented_shifts(two_cut):
    dst, src, _patterns, _centres, _bases, found, _rows = two_cut
    events = [ScriptEvent(s, e) for s, e in cases.EVENTS]
    got = calculate_segmented_shifts(src, dst, events, cases.WINDOW, cases.PENALTY)
    assert got.shifts == found.shifts and got.segments == found.segments
    for e, k, score in zip(events, cases.TRUE_K, found.event_scores):
        assert e.shift == k / float(cases.RATE) and _bits(e.diff) == _bits(score) and not e.linked
    # a centre shift a quarter of a second off: the deltas move by it, the events land where they did
    moved = calculate_segmented_shifts(src, dst, events, cases.WINDOW, cases.PENALTY, centre_shift=0.25)
    assert [d + 0.25 for d in moved.deltas] == found.deltas and [e.shift for e in events] == found.deltas
    with pytest.raises(SushiError):
        calculate_segmented_shifts(src, dst, [ScriptEvent(5.0, 5.0)], cases.WINDOW, cases.PENALTY)
    with pytest.raises(SushiError):
        calculate_segmented_shifts(src, dst, [], cases.WINDOW, cases.PENALTY)
