"""The joint search on the GPU: sushi_hip_joint_reduce against its NumPy restatement (sushi_amd/joint.py joint_host), bit for bit, on
synthetic rows; WavStream.find_joint / find_joint_many against the CPU oracle's rows and against lone searches; stream ends,
chunking, the decoy scenario of tests/test_joint_host.py, and shifts.calculate_group_shifts."""
import numpy as np
import pytest

import joint_cases as cases
from sushi_amd import joint, synth
from sushi_amd.common import SushiError
from sushi_amd.shifts import ScriptEvent, calculate_group_shifts
from sushi_amd.wav import WavStream

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")
RATE = 12000
PLANTED = 2.5


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host(curves, rows, groups, method):
    return [joint.joint_host([curves[o:o + n] for o, _w in rows[first:first + m]], [w for _o, w in rows[first:first + m]], method)
            for first, m, n in groups]


def _assert_equals_host(res, want, groups, with_curve):
    idx, score, row_score, row_idx, row_best = (t.cpu().numpy() for t in res[:5])
    joint_rows = res.joint.cpu().numpy() if with_curve else None
    assert res.joint_offsets.tolist() == np.concatenate(([0], np.cumsum([n for _f, _m, n in groups]))).tolist()
    for g, ((first, m, n), w) in enumerate(zip(groups, want)):
        assert idx[g] == w.index and _bits(score[g]) == _bits(w.score), (g, m, n, idx[g], w.index)
        assert (_bits(row_score[first:first + m]) == _bits(w.row_scores)).all(), (g, m, n)
        assert (row_idx[first:first + m] == w.row_own_index).all(), (g, m, n)
        assert (_bits(row_best[first:first + m]) == _bits(w.row_own_scores)).all(), (g, m, n)
        if with_curve:
            a = int(res.joint_offsets[g])
            assert (_bits(joint_rows[a:a + n]) == _bits(w.joint)).all(), (g, m, n)


# ---------------------------------------------------------------------------------------------- the reduce, synthetic rows
@pytest.fixture(scope="module", params=METHODS)
def ragged(request):
    curves, rows, groups = cases.ragged_groups(request.param, seed=3)
    return request.param, curves, rows, groups, _host(curves, rows, groups, request.param)


def test_reduce_equals_joint_host_on_ragged_groups(ragged):
    """(rows, shifts) of one call: (1, 1) (2, 63) (7, 64) (9, 65) (33, 1023) (3, 4097) (16, 70001); rows of different groups
    interleaved at odd offsets; weights 1/m, 1/3 and 0; a tie across a workgroup boundary, one in the last element, an all-ones
    group; with and without the joint rows."""
    import torch
    method, curves, rows, groups, want = ragged
    by_shape = {(m, n): g for g, (_f, m, n) in enumerate(groups)}
    assert want[by_shape[(33, 1023)]].index == 511 and want[by_shape[(3, 4097)]].index == 4095 and want[by_shape[(9, 65)]].index == 0
    assert all(o % 2 == 1 for o, _w in rows)
    dev = torch.from_numpy(curves).cuda()
    with_rows = joint.joint_reduce_device(dev, rows, groups, method, with_curve=True)
    _assert_equals_host(with_rows, want, groups, True)
    without = joint.joint_reduce_device(dev, rows, groups, method)
    assert without.joint is None
    _assert_equals_host(without, want, groups, False)


def test_two_calls_on_two_streams(ragged):
    import torch
    method, curves, rows, groups, want = ragged
    dev = torch.from_numpy(curves).cuda()
    # the second call's tables: the same groups backwards (another upload, another workspace)
    order = list(range(len(groups)))[::-1]
    rows2, groups2, want2 = [], [], []
    for g in order:
        first, m, n = groups[g]
        groups2.append((len(rows2), m, n))
        rows2 += rows[first:first + m]
        want2.append(want[g])
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    a = joint.joint_reduce_device(dev, rows, groups, method, with_curve=True, hip_stream=s1.cuda_stream)
    b = joint.joint_reduce_device(dev, rows2, groups2, method, with_curve=True, hip_stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    _assert_equals_host(a, want, groups, True)
    _assert_equals_host(b, want2, groups2, True)


@pytest.mark.parametrize("method", METHODS)
def test_reduce_with_large_items(method):
    """2048 items of 2048 shifts: the size from which on a workgroup takes eight indices per thread; the last item is cut short,
    and a small group rides along."""
    import torch
    rng = np.random.default_rng(17)
    n_big = 2048 * 2047 + 77
    curves = rng.random(2 * n_big + 3 * 100 + 16, dtype=np.float32) * np.float32(0.5) + np.float32(0.25 if method == "sqdiff_normed" else -0.5)
    rows = [(1, 0.5), (n_big + 4, 1.0 / 3.0), (2 * n_big + 5, 1.0 / 3.0), (2 * n_big + 106, 0.0), (2 * n_big + 207, 1.0 / 3.0)]
    groups = [(0, 2, n_big), (2, 3, 100)]
    best = np.float32(0.125 if method == "sqdiff_normed" else 0.875)
    curves[1 + n_big - 1] = curves[n_big + 4 + n_big - 1] = best           # the extremum in the cut item's last element
    want = _host(curves, rows, groups, method)
    assert want[0].index == n_big - 1
    res = joint.joint_reduce_device(torch.from_numpy(curves).cuda(), rows, groups, method, with_curve=True)
    _assert_equals_host(res, want, groups, True)


# ---------------------------------------------------------------------------------------------- find_joint_many
def _streams(sample_type):
    dst_pcm = synth.make_dst_pcm(40, RATE, seed=31)
    src_pcm = synth.make_src_pcm(dst_pcm, int(PLANTED * RATE), seed=32)
    return (WavStream.from_samples(dst_pcm, RATE, sample_type=sample_type), WavStream.from_samples(src_pcm, RATE, sample_type=sample_type))


# source spans of the events; centres a multiple of 1/8 s (exact at 12 kHz) off the true place, so that a lone find_substreams call
# over the same centre and size covers exactly the joint range
FIVE = [(5.0, 5.5), (6.25, 6.75), (8.0, 8.625), (9.5, 9.875), (11.0, 11.75)]
ONE = [(20.0, 20.5)]
OFF_CENTRE = 0.125


def _group(src, spans):
    return [src.get_substream(s, e) for s, e in spans], [s + PLANTED + OFF_CENTRE for s, _e in spans]


@pytest.fixture(scope="module")
def u8_case(oracle):
    dst, src = _streams("uint8")
    groups = [_group(src, FIVE), _group(src, ONE)]
    sizes = [3.0, 1.0]
    found = dst.find_joint_many(groups, sizes, with_curve=True)
    want = []
    for (patterns, centres), size in zip(groups, sizes):
        bases = [dst._get_sample_for_time(c) for c in centres]
        k_lo, n = joint.joint_window(bases, [p.shape[1] for p in patterns], dst.data.shape[1], int(RATE * size))
        rows = cases.oracle_rows(oracle, dst, patterns, bases, k_lo, n)
        want.append((k_lo, n, joint.joint_host(rows, [1.0 / len(rows)] * len(rows))))
    return dst, src, groups, sizes, found, want


def test_find_joint_many_u8_equals_the_oracle(u8_case):
    _dst, _src, groups, sizes, found, want = u8_case
    assert len(found) == 2
    for match, (k_lo, n, w), size in zip(found, want, sizes):
        assert (match.k_lo, match.n_shift) == (k_lo, n) == (-int(RATE * size), 2 * int(RATE * size) + 1)
        assert match.index == w.index and _bits(match.score) == _bits(w.score)
        assert (_bits(match.event_scores) == _bits(w.row_scores)).all()
        assert (_bits(match.curve) == _bits(w.joint)).all()
        assert match.delta == (k_lo + w.index) / float(RATE) == -OFF_CENTRE              # the planted place
        assert [round(d * RATE) - k_lo for d in match.event_own_delta] == w.row_own_index.tolist()
        assert (_bits(match.event_own_scores) == _bits(w.row_own_scores)).all()


def test_event_own_results_are_the_lone_searches(u8_case):
    dst, _src, groups, sizes, found, _want = u8_case
    for (patterns, centres), size, match in zip(groups, sizes, found):
        scores, _times, index = dst.find_substreams(patterns, centres, [size] * len(patterns), with_index=True)
        bases = [dst._get_sample_for_time(c) for c in centres]
        assert [b + round(d * RATE) for b, d in zip(bases, match.event_own_delta)] == index
        assert (_bits(match.event_own_scores) == _bits(scores)).all()


def test_chunked_run_gives_the_same_bits(u8_case):
    dst, _src, groups, sizes, found, _want = u8_case
    need = [4 * len(p) * m.n_shift for (p, _c), m in zip(groups, found)]
    chunked = dst.find_joint_many(groups, sizes, with_curve=True, max_bytes=need[0] + need[1] - 1)      # one group per chunk
    for a, b in zip(found, chunked):
        assert (a.index, a.delta, a.k_lo, a.n_shift, a.event_own_delta) == (b.index, b.delta, b.k_lo, b.n_shift, b.event_own_delta)
        for name in ("score", "event_scores", "event_own_scores", "curve"):
            assert (_bits(getattr(a, name)) == _bits(getattr(b, name))).all(), name
    with pytest.raises(SushiError) as e:
        dst.find_joint_many(groups, sizes, max_bytes=need[0] - 1)
    assert str(need[0]) in str(e.value)


def test_weights_and_method(u8_case):
    dst, _src, groups, sizes, found, _want = u8_case
    patterns, centres = groups[0]
    lens = [p.shape[1] for p in patterns]
    by_length = dst.find_joint(patterns, centres, sizes[0], weights="length", with_curve=True)
    explicit = dst.find_joint(patterns, centres, sizes[0], weights=[float(n) / sum(lens) for n in lens], with_curve=True)
    assert by_length.index == explicit.index == found[0].index and (_bits(by_length.curve) == _bits(explicit.curve)).all()
    assert (_bits(by_length.curve) != _bits(found[0].curve)).any()
    rows = dst.match_templates(patterns, centres, [sizes[0]] * len(patterns), method="ccoeff_normed")
    want = joint.joint_host([r[0] for r in rows], [0.2] * 5, "ccoeff_normed")
    got = dst.find_joint(patterns, centres, sizes[0], method="ccoeff_normed")
    assert got.index == want.index == found[0].index and _bits(got.score) == _bits(want.score)
    assert (_bits(got.event_scores) == _bits(want.row_scores)).all()
    for bad in ("median", [1.0], [[1.0] * 5, [1.0]]):
        with pytest.raises(SushiError):
            dst.find_joint(patterns, centres, sizes[0], weights=bad)


def test_find_joint_many_f32_equals_joint_host_over_match_templates():
    dst, src = _streams("float32")
    spans = FIVE[:3]
    patterns, centres = _group(src, spans)
    rows = dst.match_templates(patterns, centres, [1.0] * 3)
    want = joint.joint_host([r[0] for r in rows], [1.0 / 3] * 3)
    got = dst.find_joint(patterns, centres, 1.0, with_curve=True)
    assert got.n_shift == rows[0].shape[1] == 2 * RATE + 1
    assert got.index == want.index and _bits(got.score) == _bits(want.score) and got.delta == -OFF_CENTRE
    assert (_bits(got.event_scores) == _bits(want.row_scores)).all() and (_bits(got.curve) == _bits(want.joint)).all()
    assert [round(d * RATE) - got.k_lo for d in got.event_own_delta] == want.row_own_index.tolist()


def test_stream_ends_cut_the_joint_range(oracle, u8_case):
    dst, src = u8_case[0], u8_case[1]
    pad, total = dst.padding_size, dst.data.shape[1]
    patterns = [src.get_substream(1.0, 1.5), src.get_substream(30.0, 30.5)]
    centres = [-9.5, 49.25]                       # half a second into the left padding; a quarter in front of the last fitting place
    bases = [dst._get_sample_for_time(c) for c in centres]
    assert bases == [pad - int(9.5 * RATE), total - 6000 - 3000]
    got = dst.find_joint(patterns, centres, 1.0, with_curve=True)
    assert (got.k_lo, got.n_shift) == (-6000, 9001)
    rows = cases.oracle_rows(oracle, dst, patterns, bases, got.k_lo, got.n_shift)
    want = joint.joint_host(rows, [0.5, 0.5])
    assert got.index == want.index and _bits(got.score) == _bits(want.score) and (_bits(got.curve) == _bits(want.joint)).all()
    assert (_bits(got.event_scores) == _bits(want.row_scores)).all()
    with pytest.raises(SushiError):
        dst.find_joint(patterns, [-10.5, 49.5], 1.0)          # the first event needs k >= 6000, the second k <= 0
    with pytest.raises(SushiError):
        dst.find_joint([patterns[0], patterns[1][:, :0]], centres, 1.0)


# ---------------------------------------------------------------------------------------------- what it is for
def test_the_decoy_scenario_on_the_gpu():
    """tests/test_joint_host.py's scenario and its recorded oracle results: the lone search returns the decoy, the joint one the
    true shift."""
    dst, src = cases.decoy_streams()
    patterns = [src.get_substream(s, e) for s, e in cases.EVENTS]
    centres = [s for s, _e in cases.EVENTS]
    s = cases.EVENTS[cases.VICTIM][0]
    score, time = dst.find_substream(patterns[cases.VICTIM], s, cases.WINDOW)
    assert abs(time - (s + (cases.OFFSET + cases.DECOY) / float(cases.RATE))) < 1e-9
    assert int(_bits(score)[0]) == cases.VICTIM_LONE_SCORE_BITS
    got = dst.find_joint(patterns, centres, cases.WINDOW)
    assert (got.k_lo, got.n_shift) == (cases.K_LO, cases.N_SHIFT)
    assert got.delta == cases.JOINT_K / float(cases.RATE) and int(_bits(got.score)[0]) == cases.JOINT_SCORE_BITS
    assert _bits(got.event_scores).tolist() == cases.EVENT_SCORE_BITS
    assert [round(d * cases.RATE) for d in got.event_own_delta] == cases.LONE_K
    assert int(_bits(got.event_own_scores)[cases.VICTIM]) == cases.VICTIM_LONE_SCORE_BITS


def test_calculate_group_shifts(u8_case):
    dst, src = u8_case[0], u8_case[1]
    groups = [[ScriptEvent(s, e) for s, e in FIVE[:3]], [ScriptEvent(s, e) for s, e in FIVE[3:] + ONE]]
    matches = calculate_group_shifts(src, dst, groups, 1.5, centre_shifts=[2.0, 3.0])
    assert [m.delta for m in matches] == [0.5, -0.5]
    for group, match in zip(groups, matches):
        assert len(match.event_scores) == len(group)
        for e, score in zip(group, match.event_scores):
            assert e.shift == PLANTED and _bits(e.diff) == _bits(score) and not e.linked
    assert len(set(float(e.diff) for g in groups for e in g)) == 6              # every event its own score
    one = calculate_group_shifts(src, dst, groups[:1], 1.5, centre_shifts=2.25)
    assert one[0].delta == 0.25 and all(e.shift == PLANTED for e in groups[0])
    with pytest.raises(SushiError):
        calculate_group_shifts(src, dst, [[ScriptEvent(5.0, 5.0)]], 1.5)
    with pytest.raises(SushiError):
        calculate_group_shifts(src, dst, groups, 1.5, centre_shifts=[2.0])
