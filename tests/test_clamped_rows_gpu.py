"""Clamped score rows on the GPU: sushi_hip_rows_from_hits and sushi_hip_rows_clamp against their NumPy restatements
(sushi_amd/rows.py rows_from_hits_host, sushi_amd/axis.py clamp_rows_host), bit for bit, on the synthetic hit lists of
tests/clamped_rows_cases.py; axis.event_rows on real streams against clamp_rows_host over match_curves' rows; every find_* with
clamp= against its host restatement run on the clamped rows; a clamp nothing fails against the unclamped call; margins over two
chunks."""
import numpy as np
import pytest

import clamped_rows_cases as cases
from sushi_amd import axis, drift, joint, rows, segments, track
from sushi_amd.common import SushiError

pytestmark = pytest.mark.gpu
METHODS = ("sqdiff_normed", "ccoeff_normed")
SAMPLE_TYPES = ("uint8", "float32")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------- the kernels, synthetic hits
@pytest.mark.parametrize("which", [0, 1, 2])
def test_rows_from_hits_equals_the_restatement(which):
    """Rows of 1, 2, T - 1, T, T + 1 and 3 T + 5 floats at odd offsets in one buffer; lists that are empty, hold index 0, the last
    index, both sides of every tile boundary, every position; a capacity met exactly and exceeded by one; capacity 0; an index out of
    range, a descending pair, a negative count.  Rows and flags: bitwise the restatement's; the floats between rows: untouched."""
    import torch
    call = cases.synthetic_calls()[which]
    want, want_flags = cases.expected(call)
    out = torch.from_numpy(np.full(call["n_out"], cases.SENTINEL_BITS, np.uint32).view(np.float32).copy()).cuda()
    flags = rows.rows_from_hits_device(torch.from_numpy(call["hits"]).cuda(), torch.from_numpy(call["counts"]).cuda(), call["table"],
                                       call["f"], out)
    got = out.cpu().numpy().view(np.uint32)
    assert flags.cpu().numpy().tolist() == want_flags.tolist()
    assert (got == want.view(np.uint32)).all()
    assert (got[cases.outside_rows(call)] == cases.SENTINEL_BITS).all()
    if which == 1:
        assert want_flags.tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 0]
    if which == 2:          # capacity 0: no hit is read; what has one overflows
        assert want_flags.tolist() == [0, 1, 0] and (got[~cases.outside_rows(call)] == 0x80000000).all()


def test_rows_from_hits_device_refuses_bad_arguments():
    import torch
    call = cases.synthetic_calls()[2]
    hits, counts = torch.from_numpy(call["hits"]).cuda(), torch.from_numpy(call["counts"]).cuda()
    out = torch.zeros(call["n_out"], dtype=torch.float32, device="cuda")
    for bad in (dict(hits=hits.long()), dict(counts=counts.int()), dict(out=out[:100]), dict(out=out.double()), dict(f=float("inf")),
                dict(table=call["table"][:2]), dict(hits=hits.cpu())):
        kw = dict(hits=hits, counts=counts, table=call["table"], f=call["f"], out=out)
        kw.update(bad)
        with pytest.raises(SushiError):
            rows.rows_from_hits_device(kw["hits"], kw["counts"], kw["table"], kw["f"], kw["out"])


@pytest.mark.parametrize("method", METHODS)
def test_rows_clamp_equals_clamp_rows_host(method):
    """Rows of every size of cases.SIZES at odd offsets, the two buffers laid out differently: between buffers, then in place; values on
    both sides of f, f itself, -0.0, a NaN.  Bitwise clamp_rows_host; nothing outside the rows is written."""
    import torch
    rng = np.random.default_rng(23)
    sizes = cases.SIZES
    in_off = np.cumsum([3] + [n + n % 2 + 2 for n in sizes[:-1]])                # odd offsets
    out_off = np.cumsum([1] + [n + n % 2 + 4 for n in sizes[::-1][:-1]])[::-1]     # ... in the opposite order
    n_in, n_out = int(in_off[-1] + sizes[-1] + 5), int(out_off[0] + sizes[0] + 7)
    src = (rng.random(n_in, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    for clamp in (0.25, 0.0):
        f = axis.clamp_value(clamp, method)
        src[in_off] = f
        src[in_off[2:] + 1], src[in_off[2:] + 2] = np.float32(-0.0), np.float32(np.nan)
        table = rows.rows_table(out_off, sizes, in_off=in_off)
        out = torch.from_numpy(np.full(n_out, cases.SENTINEL_BITS, np.uint32).view(np.float32).copy()).cuda()
        got = rows.rows_clamp_device(torch.from_numpy(src).cuda(), table, method, f, out=out).cpu().numpy().view(np.uint32)
        covered = np.zeros(n_out, bool)
        for i, o, n in zip(in_off, out_off, sizes):
            assert (got[o:o + n] == _bits(axis.clamp_rows_host(src[i:i + n], clamp, method))).all(), n
            covered[o:o + n] = True
        assert (got[~covered] == cases.SENTINEL_BITS).all()
        # in place: the rows where they are, the floats between them as they were
        same = rows.rows_table(in_off, sizes, in_off=in_off)
        dev = torch.from_numpy(src.copy()).cuda()
        assert rows.rows_clamp_device(dev, same, method, f) is dev
        got = dev.cpu().numpy()
        want = src.copy()
        for i, n in zip(in_off, sizes):
            want[i:i + n] = axis.clamp_rows_host(src[i:i + n], clamp, method)
        assert (_bits(got) == _bits(want)).all()
        with pytest.raises(SushiError):         # one buffer, a row moved
            rows.rows_clamp_device(dev, table, method, f, out=dev)
        with pytest.raises(SushiError):         # views of one buffer that share floats
            rows.rows_clamp_device(dev[:n_in - 1], same, method, f, out=dev[1:])


# ---------------------------------------------------------------------------------------------- event_rows on real streams
@pytest.fixture(scope="module", params=SAMPLE_TYPES)
def material(request):
    """The scenario of tests/clamped_rows_cases.py in one sample type: its streams and events, their axis, and match_curves' whole
    rows by both methods -- formed once."""
    dst, src = cases.streams(request.param)
    patterns, centres = cases.scenario(dst, src)
    dst_dev = dst.device_stream()
    src_dev, offs, lens, _ = dst._pattern_source(patterns, dst_dev)
    ax = axis.event_axis(dst, offs, axis.pattern_lengths(lens), centres, cases.WINDOW)
    assert (ax.k_lo, ax.n_shift) == (cases.K_LO, cases.N_SHIFT)
    whole = {}
    for method in METHODS:
        curves, row_off = axis.event_curves(dst_dev, src_dev, [ax], method)
        whole[method] = curves.cpu().numpy().reshape(len(patterns), cases.N_SHIFT)
        assert row_off == [e * cases.N_SHIFT for e in range(len(patterns))]
    return dict(sample_type=request.param, dst=dst, src=src, patterns=patterns, centres=centres, dst_dev=dst_dev, src_dev=src_dev, ax=ax,
                whole=whole)


@pytest.mark.parametrize("method", METHODS)
def test_event_rows_equals_the_clamped_curves(material, method):
    """One threshold run, one fill and scatter, the overflowed event densely: bitwise clamp_rows_host of match_curves' rows.  Not
    vacuous: at least two events come from their hits, the twice-planted one overflows the explicit capacity, the absent one has no
    hit.  The default capacity holds every event's hits; capacity 0 sends every event with a hit the dense way."""
    m = material
    clamp, cap = cases.CLAMPS[method], cases.CAPACITY[method]
    f = axis.clamp_value(clamp, method)
    want = axis.clamp_rows_host(m["whole"][method], clamp, method)
    passing = [int(c) for c in ((m["whole"][method] >= f) if method == "ccoeff_normed" else (m["whole"][method] <= f)).sum(axis=1)]
    info = {}
    curves, row_off = axis.event_rows(m["dst_dev"], m["src_dev"], [m["ax"]], method, clamp=clamp, capacity=cap, info=info)
    got = curves.cpu().numpy().reshape(want.shape)
    print(m["sample_type"], method, "hits per event", passing, info)
    assert (_bits(got) == _bits(want)).all() and row_off == [e * cases.N_SHIFT for e in range(len(want))]
    assert info["n_sparse"] >= 2 and info["n_dense"] >= 1 and info["n_sparse"] + info["n_dense"] == len(want)
    assert info["hits"] == sum(passing) and info["capacity"] == cap and 0 < info["pairs_evaluated"] <= info["pairs"]
    assert passing[cases.TWICE] > cap and passing[cases.ABSENT] == 0 and (_bits(got[cases.ABSENT]) == _bits(f)).all()
    assert info["n_dense"] == sum(p > cap for p in passing)
    for capacity, n_dense in ((None, 0), (0, sum(p > 0 for p in passing))):
        info = {}
        curves, _ = axis.event_rows(m["dst_dev"], m["src_dev"], [m["ax"]], method, clamp=clamp, capacity=capacity, info=info)
        assert (_bits(curves.cpu().numpy().reshape(want.shape)) == _bits(want)).all()
        assert info["n_dense"] == n_dense and info["capacity"] == (1024 if capacity is None else 0)
    # clamp=None is event_curves
    curves, _ = axis.event_rows(m["dst_dev"], m["src_dev"], [m["ax"]], method)
    assert (_bits(curves.cpu().numpy().reshape(want.shape)) == _bits(m["whole"][method])).all()


# ---------------------------------------------------------------------------------------------- the four searches
def _true_scores(whole, index):
    return np.array([row[k] for row, k in zip(whole, index)], np.float32)


def _own(found, want_index, want_scores, k_lo):
    assert [round(d * cases.RATE) - k_lo for d in found.event_own_delta] == list(want_index)
    assert (_bits(found.event_own_scores) == _bits(want_scores)).all()


@pytest.mark.parametrize("method", METHODS)
def test_every_search_equals_its_restatement_on_the_clamped_rows(material, method):
    """find_joint, find_segments, find_drift and find_track (with margins) with clamp=: shifts, costs, curves, lines, margins and
    marginals are bitwise joint_host, path_host, drift_host, track_host and track_margins_host run on clamp_rows_host of
    match_curves' rows; event_scores are the true scores at the chosen shifts."""
    m = material
    dst, patterns, centres = m["dst"], m["patterns"], m["centres"]
    clamp, cap, E, k_lo = cases.CLAMPS[method], cases.CAPACITY[method], len(m["patterns"]), cases.K_LO
    f = axis.clamp_value(clamp, method)
    whole = m["whole"][method]
    clamped = list(axis.clamp_rows_host(whole, clamp, method))
    kw = dict(method=method, clamp=clamp, capacity=cap)

    want = joint.joint_host(clamped, [1.0 / E] * E, method)
    got = dst.find_joint(patterns, centres, cases.WINDOW, with_curve=True, **kw)
    assert got.index == want.index and _bits(got.score) == _bits(want.score) and (_bits(got.curve) == _bits(want.joint)).all()
    assert (_bits(got.event_scores) == _bits(_true_scores(whole, [want.index] * E))).all()
    _own(got, want.row_own_index, want.row_own_scores, k_lo)
    assert got.clamp == float(f) and got.rows_info["n_dense"] >= 1 and got.rows_info["formings"] == 1
    assert got.event_own_scores[cases.ABSENT] == f and got.event_own_delta[cases.ABSENT] == k_lo / float(cases.RATE)

    want = segments.path_host(clamped, [1.0] * E, cases.PENALTY, method)
    got = dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY, **kw)
    assert got.shifts == [k_lo + int(k) for k in want.shifts] and _bits64(got.cost) == _bits64(want.cost)
    assert (_bits(got.event_scores) == _bits(_true_scores(whole, want.shifts))).all()
    _own(got, want.row_own_index, want.row_own_scores, k_lo)
    assert got.clamp == float(f) and got.rows_info["n_dense"] >= 1

    got = dst.find_drift(patterns, centres, cases.WINDOW, cases.MAX_RATE, with_lines=True, **kw)
    offsets = drift.drift_offsets(m["ax"].bases, got.drift_rates)
    want = drift.drift_host(clamped, [1.0 / E] * E, offsets, method)
    assert (got.drift, got.index) == (want.drift, want.index) and _bits(got.score) == _bits(want.score)
    assert (_bits(got.drift_scores) == _bits(want.drift_scores)).all() and (_bits(got.lines) == _bits(want.lines)).all()
    assert (_bits(got.event_scores) == _bits(_true_scores(whole, [want.index + int(o) for o in offsets[want.drift]]))).all()
    own = joint.joint_host(clamped, [1.0 / E] * E, method)
    _own(got, own.row_own_index, own.row_own_scores, k_lo)
    assert got.clamp == float(f) and got.rows_info["n_dense"] >= 1

    want = track.track_margins_host(clamped, [1.0] * E, cases.PENALTY, cases.STEP_COST, cases.REACH, 120, method)
    got = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, reach=cases.REACH, step_cost=cases.STEP_COST, margins=True,
                         guard=120, marginals=True, **kw)
    assert got.shifts == [k_lo + int(k) for k in want.shifts] and _bits64(got.cost) == _bits64(want.cost)
    assert (_bits64(got.event_through) == _bits64(want.through)).all()
    assert (_bits64(got.event_margin) == _bits64(np.where(want.alt_arg == track.NO_ALT, np.inf, want.alt - want.through))).all()
    assert got.event_alt_shift == [None if int(k) == track.NO_ALT else k_lo + int(k) for k in want.alt_arg]
    assert (_bits64(got.marginals.cpu().numpy()) == _bits64(want.marginals)).all()
    assert (_bits(got.event_scores) == _bits(_true_scores(whole, want.shifts))).all()
    _own(got, want.row_own_index, want.row_own_scores, k_lo)
    assert got.clamp == float(f) and got.rows_info["formings"] == 1
    plain = dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, reach=cases.REACH, step_cost=cases.STEP_COST, **kw)
    host = track.track_host(clamped, [1.0] * E, cases.PENALTY, cases.STEP_COST, cases.REACH, method)
    assert plain.shifts == [k_lo + int(k) for k in host.shifts] and _bits64(plain.cost) == _bits64(host.cost)


def _same(a, b, skip=("clamp", "rows_info")):
    """Two result records hold the same bits in every field but `skip`."""
    assert set(a.__dict__) == set(b.__dict__)
    for name, x in a.__dict__.items():
        y = b.__dict__[name]
        if name in skip:
            continue
        if hasattr(x, "cpu"):
            x, y = x.cpu().numpy(), y.cpu().numpy()
        if isinstance(x, np.ndarray) or isinstance(x, np.generic):
            x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
        else:
            assert x == y, name


def _searches(m, method):
    dst, patterns, centres = m["dst"], m["patterns"], m["centres"]
    return [
        ("find_joint", lambda **kw: dst.find_joint(patterns, centres, cases.WINDOW, with_curve=True, method=method, **kw)),
        ("find_segments", lambda **kw: dst.find_segments(patterns, centres, cases.WINDOW, cases.PENALTY, method=method, **kw)),
        ("find_drift", lambda **kw: dst.find_drift(patterns, centres, cases.WINDOW, cases.MAX_RATE, with_lines=True, method=method, **kw)),
        ("find_track", lambda **kw: dst.find_track(patterns, centres, cases.WINDOW, cases.PENALTY, reach=cases.REACH,
                                                   step_cost=cases.STEP_COST, margins=True, marginals=True, method=method, **kw))]


@pytest.mark.parametrize("method", METHODS)
def test_a_clamp_nothing_fails_changes_no_bit(material, method):
    """clamp 3.0 ('sqdiff_normed') / -2.0 ('ccoeff_normed'): every score passes.  With room for every hit no event goes the dense
    way and every search returns the unclamped call's bits; with capacity 0 every event goes the dense way, and the bits are the
    same again."""
    clamp = cases.PASS_ALL[method]
    for name, call in _searches(material, method):
        plain = call()
        assert plain.clamp is None and plain.rows_info is None
        sparse = call(clamp=clamp, capacity=cases.N_SHIFT)
        _same(sparse, plain)
        E = len(material["patterns"])
        assert sparse.rows_info["n_dense"] == 0 and sparse.rows_info["n_sparse"] == E and sparse.rows_info["hits"] == E * cases.N_SHIFT, name
        assert sparse.clamp == clamp
        dense = call(clamp=clamp, capacity=0)
        _same(dense, plain)
        assert dense.rows_info["n_dense"] == E and dense.rows_info["n_sparse"] == 0 and dense.rows_info["capacity"] == 0, name


@pytest.mark.parametrize("method", METHODS)
def test_margins_over_two_chunks_equal_one_chunk(material, method):
    """find_track(margins=True, clamp=) with a max_bytes that holds four of the seven events: both chunks are formed twice, through
    event_rows both times, and the result is the one-chunk result bit for bit."""
    m = material
    kw = dict(reach=cases.REACH, step_cost=cases.STEP_COST, margins=True, marginals=True, method=method, clamp=cases.CLAMPS[method],
              capacity=cases.CAPACITY[method])
    one = m["dst"].find_track(m["patterns"], m["centres"], cases.WINDOW, cases.PENALTY, **kw)
    two = m["dst"].find_track(m["patterns"], m["centres"], cases.WINDOW, cases.PENALTY, max_bytes=4 * 4 * cases.N_SHIFT + 3, **kw)
    _same(two, one)
    assert one.rows_info["formings"] == 1 and two.rows_info["formings"] == 4
    assert two.rows_info["n_dense"] == 2 * one.rows_info["n_dense"] and two.rows_info["hits"] == 2 * one.rows_info["hits"]


def test_shifts_helpers_pass_clamp_through(material):
    from sushi_amd.shifts import (ScriptEvent, calculate_drifting_shifts, calculate_group_shifts, calculate_segmented_shifts,
                                  calculate_tracked_shifts)
    m, method = material, "sqdiff_normed"
    clamp, cap = cases.CLAMPS[method], cases.CAPACITY[method]
    events = [ScriptEvent(s, e) for s, e in cases.EVENTS]
    kw = dict(clamp=clamp, capacity=cap)
    found = calculate_group_shifts(m["src"], m["dst"], [events], cases.WINDOW, **kw)[0]
    _same(found, m["dst"].find_joint(m["patterns"], m["centres"], cases.WINDOW, **kw), skip=())
    found = calculate_segmented_shifts(m["src"], m["dst"], events, cases.WINDOW, cases.PENALTY, **kw)
    _same(found, m["dst"].find_segments(m["patterns"], m["centres"], cases.WINDOW, cases.PENALTY, **kw), skip=())
    assert [e.shift for e in events] == found.deltas
    found = calculate_drifting_shifts(m["src"], m["dst"], events, cases.WINDOW, cases.MAX_RATE, **kw)
    _same(found, m["dst"].find_drift(m["patterns"], m["centres"], cases.WINDOW, cases.MAX_RATE, **kw), skip=())
    found = calculate_tracked_shifts(m["src"], m["dst"], events, cases.WINDOW, cases.PENALTY, reach=cases.REACH, **kw)
    _same(found, m["dst"].find_track(m["patterns"], m["centres"], cases.WINDOW, cases.PENALTY, reach=cases.REACH, **kw), skip=())
    assert found.clamp == float(axis.clamp_value(clamp, method)) and found.rows_info["capacity"] == cap
