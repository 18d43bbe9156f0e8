"""The drift search without a GPU: the NumPy restatement of sushi_hip_drift_reduce's arithmetic (sushi_amd/drift.py drift_host), the
kernel's own header compiled for the CPU (tests/host_drift_check.cpp, a program of its own under AddressSanitizer + UBSan),
rate_grid / drift_offsets as integers, the entry points' argument checks, and the retimed scenario on the CPU oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import drift_cases as cases
import joint_cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, drift, joint
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("drift_check")), "host_drift_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_drift_check.cpp"), "-o", exe])
    return exe


def _loop(rows, weights, offsets, method):
    """The definition, written out: one candidate and one index at a time, row after row, on Python floats (IEEE float64); the
    answer by a scan in table order that only a strictly better value replaces."""
    n, better = rows[0].shape[0], (lambda v, b: v > b) if method == "ccoeff_normed" else (lambda v, b: v < b)
    lines = np.full((len(offsets), n), -np.inf if method == "ccoeff_normed" else np.inf, np.float32)
    answer, per_drift = None, []
    for d, o in enumerate(offsets):
        lo, hi = max(0, max(-int(x) for x in o)), n - max(0, max(int(x) for x in o))
        own = None
        for j in range(lo, hi):
            acc = 0.0
            for r, w, oe in zip(rows, weights, o):
                acc = acc + float(w) * float(r[j + int(oe)])
            lines[d, j] = np.float32(acc)
            if own is None or better(lines[d, j], lines[d, own]):
                own = j
        per_drift.append(own)
        if answer is None or better(lines[d, own], lines[answer[0], answer[1]]):
            answer = (d, own)
    return answer, per_drift, lines


# ---------------------------------------------------------------------------------------------- drift_host
@pytest.mark.parametrize("method", METHODS)
def test_drift_host_is_the_loop_written_out(method):
    for case in cases.grid_cases(method)[:20] + cases.special_cases(method):
        rows, weights = cases.rows_of(case)
        got = drift.drift_host(rows, weights, case.offsets, method)
        (d, j), per_drift, lines = _loop(rows, weights, case.offsets, method)
        assert (got.drift, got.index) == (d, j), case.name
        assert (_bits(got.lines) == _bits(lines)).all(), case.name
        assert got.drift_index.tolist() == per_drift and (_bits(got.drift_scores) == _bits(lines[np.arange(len(per_drift)), per_drift])).all()
        assert _bits(got.score) == _bits(lines[d, j])
        assert (_bits(got.row_scores) == _bits([r[j + int(o)] for r, o in zip(rows, case.offsets[d])])).all(), case.name
        if case.expect is not None:
            assert (got.drift, got.index) == case.expect, case.name


def test_the_cases_cover_what_they_claim():
    grid = cases.grid_cases("sqdiff_normed")
    assert {len(c.rows) for c in grid} == set(cases.ROWS) and {c.n_shift for c in grid} == set(cases.SHIFTS)
    for n in cases.SHIFTS:
        assert {c.offsets.shape[0] for c in grid if c.n_shift == n} == set(cases.DRIFTS), n
    kinds = set()
    for c in grid:
        assert all(o % 2 == 1 for o, _w in c.rows)
        kinds.add(("zero" if not c.offsets.any() else "negative" if (c.offsets <= 0).all() else
                   "positive" if (c.offsets >= 0).all() else "mixed"))
    assert kinds == set(cases.KINDS) and any(w == 0.0 for c in grid for _o, w in c.rows)
    special = {c.name: c for c in cases.special_cases("ccoeff_normed")}
    _o, lo, hi = drift.checked_offsets(special["single_index_range"].offsets, 3, 65)
    assert (lo[1], hi[1]) == (30, 31)
    _o, lo, hi = drift.checked_offsets(special["range_ends_in_last_item"].offsets, 4, 1200)
    assert hi.tolist() == [1100, 1200, 1190] and 1024 < hi[0] < 1200
    zeros = special["signed_zeros"]
    got = drift.drift_host(*cases.rows_of(zeros), zeros.offsets, "ccoeff_normed")
    assert _bits(got.row_scores).tolist() == [0x80000000, 0] and int(_bits(got.score)[0]) == 0     # a line's value is never -0.0
    assert (got.drift_scores[1:] == 0.0).all() and got.drift_index.tolist()[1:] == [20, 20, 21]


def test_drift_with_one_candidate_of_zeros_is_the_joint_search():
    case = cases.grid_cases("sqdiff_normed")[7]
    rows, weights = cases.rows_of(case)
    a = drift.drift_host(rows, weights, np.zeros((1, len(rows)), np.int32))
    b = joint.joint_host(rows, weights)
    assert (a.drift, a.index) == (0, b.index) and _bits(a.score) == _bits(b.score)
    assert (_bits(a.lines[0]) == _bits(b.joint)).all() and (_bits(a.row_scores) == _bits(b.row_scores)).all()


def test_drift_host_refuses_bad_arguments():
    r = np.zeros(4, np.float32)
    zero = np.zeros((1, 1), np.int32)
    for rows, weights, offsets in (([], [], zero), ([r], [1.0, 1.0], zero), ([r], [-1.0], zero), ([r], [float("nan")], zero),
                                   ([r.astype(np.float64)], [1.0], zero), ([r], [1.0], np.zeros((0, 1), np.int32)),
                                   ([r], [1.0], np.zeros((1, 2), np.int32)), ([r], [1.0], np.zeros(1, np.int32)),
                                   ([r], [1.0], np.zeros((1, 1), np.float64)), ([r], [1.0], np.zeros((65536, 1), np.int32)),
                                   ([r], [1.0], [[4]]), ([r], [1.0], [[-4]]), ([r, r], [1.0, 1.0], [[2, -2]]),
                                   ([r], [1.0], [[2 ** 31]]), ([r], [1.0], [[-2 ** 31 - 1]])):
        with pytest.raises(SushiError):
            drift.drift_host(rows, weights, offsets)
    with pytest.raises(SushiError):
        drift.drift_host([r], [1.0], zero, "sqdiff")
    assert drift.drift_host([r, r], [1.0, 1.0], [[2, -1]]).index == 1           # reach 3 < 4: the single index 1


# ---------------------------------------------------------------------------------------------- the kernel's header on the CPU
EXPECTED_RC = {   # case of host_drift_check validate -> what stage_drift returns
    "good": 0, "good_ccoeff": 0, "method_2": -1, "method_neg": -1, "null_rows": -1, "null_offsets": -1, "no_rows": -1,
    "negative_rows": -1, "no_drifts": -1, "negative_drifts": -1, "drifts_65536": -1, "drifts_int32_max": -1, "no_shift": -1,
    "negative_shift": -1, "empty_curves": -1, "negative_curves": -1, "shift_beyond_curves": -1, "row_before_curves": -1,
    "row_ends_at_curves_end": 0, "row_one_past_curves_end": -1, "row_at_int64_max": -1, "row_sum_overflows": -1,
    "huge_curves_row_at_end": 0, "huge_curves_row_past_end": -1, "weight_nan": -1, "weight_inf": -1, "weight_neg_inf": -1,
    "weight_negative": -1, "weight_neg_zero": 0, "weight_large": 0, "offset_minus_n_shift": -1, "offset_n_shift": -1,
    "reach_is_n_shift": -1, "reach_is_n_shift_above": -1, "offset_int32_min": -1, "offset_int32_max": -1,
    "offsets_int32_min_and_max": -1, "one_shift_offsets_not_zero": -1, "one_shift_offsets_zero": 0,
    "int32_max_shifts_single_index": 0, "int32_max_shifts_empty": -1, "bad_candidate_behind_n_drifts": 0,
    "bad_candidate_not_counted": 0}


def _layout_bytes(n_rows, n_drifts):
    up = lambda b: (b + 255) // 256 * 256
    slots = (n_drifts + cases.DB - 1) // cases.DB * cases.DB
    return up(16 * n_rows) + up(4 * slots * n_rows) + up(8 * slots) + up(8 * slots) + 256


def test_stage_drift_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = dict(l.split() for l in lines[:len(EXPECTED_RC)])
    assert {k: int(v) for k, v in got.items()} == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    # the rows, the offsets in blocks of DB candidates, their ranges, their keys, the answer's key: each padded to 256 bytes
    assert rest[0] == "bytes %d %d %d 0 0 0 0" % (_layout_bytes(1, 1), _layout_bytes(3, 6), _layout_bytes(64, 8641))
    # six candidates over 93 shifts: one item of 512 indices x three blocks; three candidates of a single index
    assert rest[1] == ("facts_good rc=0 per=2 jitems=1 items=3 grid=3 bytes=%d r0=[0,93) r1=[3,91) r2=[0,84) r3=[92,93) r4=[0,1) "
                       "r5=[46,47) rows_ok=1 offs_ok=1 pad_ok=1 keys_ok=1" % _layout_bytes(3, 6))
    # 8 items of 2048 shifts x 256 blocks: from 2048 such items on they are taken; one block fewer: four times the items of 512
    assert rest[2].startswith("facts_large_items rc=0 per=8 jitems=8 items=2048 grid=2048 ")
    assert rest[3].startswith("facts_small_items rc=0 per=2 jitems=32 items=8160 grid=2048 ")
    assert rest[4].startswith("facts_int32_max rc=0 per=8 jitems=1048576 items=34359738368 grid=2048 ")
    assert all(l.endswith("rows_ok=1 offs_ok=1 pad_ok=1 keys_ok=1") for l in rest[1:5]) and len(rest) == 5


def _run_check(check, tmp_path, method, case):
    rt = np.array(case.rows, dtype=_native.JOINT_ROW_DTYPE)
    paths = [os.path.join(str(tmp_path), name) for name in ("curves", "rows", "offsets", "out")]
    for p, a in zip(paths, (case.curves, rt, np.ascontiguousarray(case.offsets, np.int32))):
        a.tofile(p)
    subprocess.check_call([check, "reduce", method.split("_")[0], str(case.n_shift)] + paths)
    raw = np.fromfile(paths[3], np.uint32)
    E, D = len(case.rows), case.offsets.shape[0]
    cuts = np.cumsum([0, 2, 1, E, D, D])
    best, score, row_score, drift_idx, drift_score = (raw[a:b] for a, b in zip(cuts[:-1], cuts[1:]))
    return best.view(np.int32), score, row_score, drift_idx.view(np.int32), drift_score, raw[cuts[-1]:].reshape(D, case.n_shift)


def _compare_with_drift_host(got, case, method):
    best, score, row_score, drift_idx, drift_score, lines = got
    want = drift.drift_host(*cases.rows_of(case), case.offsets, method)
    assert best.tolist() == [want.drift, want.index] and score[0] == _bits(want.score), case.name
    assert (row_score == _bits(want.row_scores)).all(), case.name
    assert (drift_idx == want.drift_index).all() and (drift_score == _bits(want.drift_scores)).all(), case.name
    assert (lines == _bits(want.lines)).all(), case.name
    if case.expect is not None:
        assert tuple(best.tolist()) == case.expect, case.name


@pytest.mark.parametrize("method", METHODS)
def test_the_header_on_the_cpu_equals_drift_host(check, tmp_path, method):
    """drift_value, the staged ranges and the first-extremum rule of drift_core.hpp, run by a program of its own over the cases of
    the GPU test (tests/drift_cases.py)."""
    for case in cases.grid_cases(method) + cases.special_cases(method) + [cases.large_case(method)]:
        _compare_with_drift_host(_run_check(check, tmp_path, method, case), case, method)


def test_the_header_on_the_cpu_on_cases_written_here(check, tmp_path):
    # the order-dependent sum (2^60 swallows the ones before it), the sum a fused multiply-add would change ((1/3) * 3 - 1)
    big = np.float32(2.0 ** 60)
    curves = np.array([1, 1, 3, 1, big, big, big, big, -big, -big, -big, -big, -1, -1, -1, 3, 3, 3], np.float32)
    swallowed = cases.Case("swallowed", curves, [(0, 1.0), (4, 1.0), (8, 1.0)], 4, np.array([[0, 0, 0], [1, -1, 0]], np.int32), None)
    plain = cases.Case("plain", curves, [(12, 1.0), (15, 1.0 / 3.0)], 3, np.array([[0, 0], [1, -1], [-2, 0]], np.int32), None)
    for method in METHODS:
        for case in (swallowed, plain):
            got = _run_check(check, tmp_path, method, case)
            _compare_with_drift_host(got, case, method)
            valid = got[5] != _bits(np.float32(np.inf if method == "sqdiff_normed" else -np.inf))
            assert not got[5][valid].any() and valid.sum() == (6 if case is swallowed else 5)


# ---------------------------------------------------------------------------------------------- rates and offsets: numbers only
def test_rate_grid():
    rates = drift.rate_grid(1e-3, 330000, 1.0)
    assert rates.shape == (661,) and rates[330] == 0.0 and (np.diff(rates) > 0).all()
    assert rates[0] == -330 * (1.0 / 330000) and rates[-1] == 330 * (1.0 / 330000)
    # one step moves the farthest event by `resolution` samples
    assert np.rint(rates * 330000.0).astype(np.int64).tolist() == list(range(-330, 331))
    half = drift.rate_grid(1e-3, 330000, 0.5)
    assert half.shape == (1321,) and np.rint(half * 330000.0 * 2).astype(np.int64).tolist() == list(range(-660, 661))
    assert drift.rate_grid(1e-4, 43200000).shape == (8641,)                     # 100 ppm over two hours at 12 kHz
    assert drift.rate_grid(0.0, 1000).tolist() == [0.0] and drift.rate_grid(1e-3, 0).tolist() == [0.0]
    assert drift.rate_grid(1e-3, 999).shape == (3,) and drift.rate_grid(1e-3, 1000).shape == (3,) and drift.rate_grid(1e-3, 1001).shape == (5,)
    with pytest.raises(SushiError) as e:
        drift.rate_grid(1e-3, 43200000)
    assert "86401" in str(e.value)
    assert drift.rate_grid(1e-3, 43200000, resolution=8.0).shape == (10801,)
    with pytest.raises(SushiError) as e:
        drift.rate_grid(1e-3, 330000, max_drifts=660)
    assert "661" in str(e.value)
    for bad in ((-1e-3, 10, 1.0), (1e-3, -1, 1.0), (1e-3, 10, 0.0), (float("nan"), 10, 1.0), (1e-3, float("inf"), 1.0)):
        with pytest.raises(SushiError):
            drift.rate_grid(*bad)


def test_drift_offsets():
    positions = [1000, 4000, 9001]
    assert drift.drift_anchor(positions) == 5000 and drift.drift_anchor([7]) == 7 and drift.drift_anchor([-3, 0]) == -2
    rates = drift.rate_grid(1e-3, 4001)
    assert rates.shape == (11,)
    o = drift.drift_offsets(positions, rates)
    assert o.dtype == np.int32 and o.shape == (11, 3)
    assert o[:, 2].tolist() == list(range(-5, 6)) and o[:, 0].tolist() == [-x for x in o[:, 2].tolist()]       # +-4000 / 4001 of a step
    assert o[5].tolist() == [0, 0, 0] and o[:, 1].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, -1, -1, -1]
    for d, r in enumerate(rates):
        assert o[d].tolist() == [int(np.rint(r * float(p - 5000))) for p in positions]
    # rint: halves go to the even neighbour, on both sides of zero
    assert drift.drift_offsets([0, 2, 5, 7], [0.5, -0.5], anchor=2).tolist() == [[-1, 0, 2, 2], [1, 0, -2, -2]]
    assert drift.drift_offsets([10, 20], [0.25], anchor=0).tolist() == [[2, 5]]
    # events clustered at the anchor give neighbouring candidates the same offsets
    near = drift.drift_offsets([5000, 5001, 4999], drift.rate_grid(1e-3, 4001))
    assert not near.any()
    with pytest.raises(SushiError):
        drift.drift_offsets([0, 2 ** 40], [1.0])
    with pytest.raises(SushiError):
        drift.drift_offsets([], [1.0])
    with pytest.raises(SushiError):
        drift.drift_offsets([1], [float("nan")])


# ---------------------------------------------------------------------------------------------- the entry points, no GPU
def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    assert {"sushi_hip_drift_bytes", "sushi_hip_drift_reduce"} <= set(_native.declared_symbols())
    assert L.sushi_hip_drift_bytes(1, 1) == _layout_bytes(1, 1) and L.sushi_hip_drift_bytes(64, 8641) == _layout_bytes(64, 8641)
    assert L.sushi_hip_drift_bytes(3, 65535) == _layout_bytes(3, 65535)
    assert L.sushi_hip_drift_bytes(0, 5) == 0 and L.sushi_hip_drift_bytes(5, 0) == 0 and L.sushi_hip_drift_bytes(5, 65536) == 0
    rows = np.array([(0, 0.5), (7, 0.5), (907, 1.0)], dtype=_native.JOINT_ROW_DTYPE)
    offsets = np.array([[0, 0, 0], [-3, 2, 0], [-46, 46, 0]], np.int32)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first

    def call(curves=P, n_curve=1000, rows=rows, n_rows=3, n_shift=93, offsets=offsets, n_drifts=3, method=0, mem=P,
             mem_bytes=1 << 16, outs=(P, P, P, P, P), lines=None):
        return L.sushi_hip_drift_reduce(curves, n_curve, None if rows is None else rows.ctypes.data, n_rows, n_shift,
                                        None if offsets is None else offsets.ctypes.data, n_drifts, method, mem, mem_bytes,
                                        *outs, lines, None)

    EINVAL, EALIGN = -1, -2
    assert call(curves=None) == EINVAL and call(rows=None) == EINVAL and call(offsets=None) == EINVAL and call(mem=None) == EINVAL
    for k in range(5):
        assert call(outs=tuple(None if i == k else P for i in range(5))) == EINVAL
    assert call(method=2) == EINVAL and call(method=-1) == EINVAL
    assert call(n_rows=0) == EINVAL and call(n_drifts=0) == EINVAL and call(n_drifts=65536) == EINVAL and call(n_shift=0) == EINVAL
    assert call(n_curve=999) == EINVAL and call(n_shift=94) == EINVAL
    for at, value in (((2, 0), -47), ((1, 1), 93), ((0, 2), -93), ((1, 0), -2 ** 31), ((1, 1), 2 ** 31 - 1)):
        bad = offsets.copy()
        bad[at] = value
        assert call(offsets=bad) == EINVAL, (at, value)
    for field, at, value in (("curve_off", 0, -1), ("curve_off", 2, 908), ("curve_off", 2, 2 ** 63 - 1), ("weight", 0, np.nan),
                             ("weight", 1, np.inf), ("weight", 2, -1.0)):
        bad = rows.copy()
        bad[field][at] = value
        assert call(rows=bad) == EINVAL, (field, at, value)
    assert call(mem=ctypes.c_void_p((1 << 20) + 128)) == EALIGN
    assert call(curves=ctypes.c_void_p((1 << 20) + 2)) == EALIGN
    assert call(lines=ctypes.c_void_p((1 << 20) + 1)) == EALIGN
    assert call(outs=(P, ctypes.c_void_p((1 << 20) + 2), P, P, P)) == EALIGN
    assert call(mem_bytes=_layout_bytes(3, 3) - 1) == _native.ENOSPACE and call(mem_bytes=0) == _native.ENOSPACE


# ---------------------------------------------------------------------------------------------- the retimed scenario on the oracle
def test_a_line_finds_the_rate_of_a_retimed_source(oracle):
    """tests/drift_cases.py's scenario with the CPU oracle's rows through drift_host: the rate is found to a grid step, and every
    event lands within EVENT_TOLERANCE samples of its own minimum near its true place -- the derivation of that bound, checked
    here before the GPU test relies on it."""
    dst, src = cases.drift_streams()
    patterns = [src.get_substream(s, s + cases.EVENT_LENGTH) for s in cases.EVENT_STARTS]
    bases = [dst._get_sample_for_time(s) for s in cases.EVENT_STARTS]
    k_lo, n_shift = joint.joint_window(bases, [p.shape[1] for p in patterns], dst.data.shape[1], int(cases.RATE * cases.WINDOW))
    assert (k_lo, n_shift) == (-6000, 12001)
    rows = joint_cases.oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift)
    anchor = drift.drift_anchor(bases)
    half_span = max(max(bases) - anchor, anchor - min(bases))
    rates = drift.rate_grid(cases.MAX_RATE, half_span)
    assert rates.shape[0] == 661
    offsets = drift.drift_offsets(bases, rates, anchor)
    got = drift.drift_host(rows, [1.0 / 12] * 12, offsets)
    step = rates[1] - rates[0]
    print("rate %.9g (true %.9g, step %.3g), index %d, score %.6g" % (rates[got.drift], cases.TRUE_RATE, step, got.index, got.score))
    assert abs(rates[got.drift] - cases.TRUE_RATE) <= step
    worst = 0
    for e, start in enumerate(cases.EVENT_STARTS):
        on_line = bases[e] + k_lo + got.index + int(offsets[got.drift][e])
        centre = int(round(cases.true_place(dst, start))) - bases[e] - k_lo
        near = rows[e][centre - cases.NEIGHBOURHOOD:centre + cases.NEIGHBOURHOOD + 1]
        own = bases[e] + k_lo + centre - cases.NEIGHBOURHOOD + oracle.argmin_first(near)
        print("event %2d: on the line %d, own minimum %d, true place %.2f" % (e, on_line, own, cases.true_place(dst, start)))
        worst = max(worst, abs(on_line - own))
    assert worst <= cases.EVENT_TOLERANCE
    # what a constant shift gives: the middle right, both ends wrong, and a worse score
    const = joint.joint_host(rows, [1.0 / 12] * 12)
    assert got.score < const.score
    assert got.row_scores[0] < const.row_scores[0] and got.row_scores[-1] < const.row_scores[-1]
