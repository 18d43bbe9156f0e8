"""The joint search without a GPU: the NumPy restatement of sushi_hip_joint_reduce's arithmetic (sushi_amd/joint.py joint_host), the
kernel's own header compiled for the CPU (tests/host_joint_check.cpp, a program of its own under AddressSanitizer + UBSan),
joint_window, the entry points' argument checks, and the decoy scenario on the CPU oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import joint_cases as cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, joint
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("joint_check")), "host_joint_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_joint_check.cpp"), "-o", exe])
    return exe


def _loop(rows, weights):
    """The definition, written out: one joint index at a time, row after row, on Python floats (IEEE float64)."""
    out = np.empty(rows[0].shape[0], np.float32)
    for j in range(out.shape[0]):
        acc = 0.0
        for r, w in zip(rows, weights):
            acc = acc + float(w) * float(r[j])
        out[j] = np.float32(acc)
    return out


def _first(row, method):
    at = 0
    for j in range(1, row.shape[0]):
        if (row[j] > row[at]) if method == "ccoeff_normed" else (row[j] < row[at]):
            at = j
    return at


def _rows(m, n, seed, method="sqdiff_normed"):
    rng = np.random.default_rng(seed)
    lo = 0.0 if method == "sqdiff_normed" else -1.0
    return [(rng.random(n, dtype=np.float32) * np.float32(1.0 - lo) + np.float32(lo)).astype(np.float32) for _ in range(m)]


# ---------------------------------------------------------------------------------------------- joint_host
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("m", [1, 2, 7, 33])
@pytest.mark.parametrize("n", [1, 63, 65, 1025])
def test_joint_host_is_the_loop_written_out(m, n, method):
    rows = _rows(m, n, seed=m * 10007 + n, method=method)
    for weights in ([1.0 / m] * m, [1.0 / 3.0] * m, [(1.0 / 3.0, 0.0)[i % 2] for i in range(m)]):
        got = joint.joint_host(rows, weights, method)
        want = _loop(rows, weights)
        assert (_bits(got.joint) == _bits(want)).all()
        at = _first(want, method)
        assert got.index == at and _bits(got.score) == _bits(want[at])
        assert (_bits(got.row_scores) == _bits([r[at] for r in rows])).all()
        own = [_first(r, method) for r in rows]
        assert got.row_own_index.tolist() == own
        assert (_bits(got.row_own_scores) == _bits([r[k] for r, k in zip(rows, own)])).all()


def test_the_sum_is_taken_in_row_order():
    """Values whose float64 sum depends on the order: 2^60 swallows the ones that came before it, and its negative then leaves 0;
    taken backwards the two cancel first and the ones survive."""
    n = 65
    ones = np.ones(n, np.float32)
    ones[7] = 3.0
    rows = [ones, np.full(n, np.float32(2.0 ** 60)), np.full(n, np.float32(-2.0 ** 60))]
    weights = [1.0, 1.0, 1.0]
    got = joint.joint_host(rows, weights)
    assert (_bits(got.joint) == _bits(_loop(rows, weights))).all() and not got.joint.any()
    backwards = _loop(rows[::-1], weights)
    assert (_bits(got.joint) != _bits(backwards)).all() and backwards[7] == 3.0
    # product and sum round separately: (1/3) * 3 rounds to 1 and 1 - 1 is 0; a fused multiply-add would leave -2^-54
    plain = joint.joint_host([np.full(4, np.float32(-1.0)), np.full(4, np.float32(3.0))], [1.0, 1.0 / 3.0])
    assert _bits(plain.joint).tolist() == [0] * 4


@pytest.mark.parametrize("method", METHODS)
def test_ties_take_the_first_index(method):
    best = np.float32(0.0 if method == "sqdiff_normed" else 1.0)
    rows = _rows(3, 65, seed=9, method=method)
    rows = [np.clip(r, np.float32(0.01), np.float32(0.99)) if method == "sqdiff_normed" else np.clip(r, np.float32(-0.9), np.float32(0.9))
            for r in rows]
    for r in rows:
        r[[20, 41, 64]] = best
    got = joint.joint_host(rows, [1.0 / 3.0] * 3, method)
    assert got.index == 20 and got.row_own_index.tolist() == [20, 20, 20]
    flat = [np.ones(63, np.float32)] * 2
    got = joint.joint_host(flat, [0.5, 0.5], method)
    assert got.index == 0 and got.row_own_index.tolist() == [0, 0] and float(got.score) == 1.0


def test_signed_zeros_tie_under_ccoeff():
    """0.0 and -0.0 compare equal: the first of them is the maximum, and its own bits are what is returned."""
    a = np.array([-0.5, -0.0, 0.0, -0.0], np.float32)
    b = np.array([-0.5, 0.0, -0.0, 0.0], np.float32)
    got = joint.joint_host([a, b], [0.5, 0.5], "ccoeff_normed")
    assert got.index == 1 and got.row_own_index.tolist() == [1, 1]
    assert _bits(got.row_own_scores).tolist() == [0x80000000, 0x00000000]
    assert _bits(got.row_scores).tolist() == [0x80000000, 0x00000000]
    assert int(_bits(got.score)[0]) == 0                                  # 0.0 + 0.5 * -0.0 = 0.0: a joint value is never -0.0
    assert _bits(got.joint).tolist() == _bits(_loop([a, b], [0.5, 0.5])).tolist()


def test_joint_host_refuses_bad_arguments():
    r = np.zeros(4, np.float32)
    for rows, weights in (([], []), ([r], [1.0, 1.0]), ([r, np.zeros(5, np.float32)], [1, 1]), ([r.astype(np.float64)], [1.0]),
                          ([np.zeros(0, np.float32)], [1.0]), ([r], [-1.0]), ([r], [float("nan")]), ([r], [float("inf")]),
                          ([r.reshape(1, 4)], [1.0])):
        with pytest.raises(SushiError):
            joint.joint_host(rows, weights)
    with pytest.raises(SushiError):
        joint.joint_host([r], [1.0], "sqdiff")


# ---------------------------------------------------------------------------------------------- the kernel's header on the CPU
EXPECTED_RC = {   # case of host_joint_check validate -> what stage_joint returns
    "good": 0, "good_ccoeff": 0, "method_2": -1, "method_neg": -1, "no_groups": -1, "no_rows": -1, "negative_counts": -1,
    "fewer_rows_than_groups": -1, "empty_curves": -1, "negative_curves": -1, "group_overlaps": -1, "group_gap": -1,
    "first_group_not_at_0": -1, "groups_out_of_order": -1, "group_without_rows": -1, "group_negative_rows": -1, "rows_left_over": -1,
    "rows_missing": -1, "rows_int32_max": -1, "no_shift": -1, "negative_shift": -1, "shift_beyond_curves": -1, "row_before_curves": -1,
    "row_ends_at_curves_end": 0, "row_one_past_curves_end": -1, "single_shift_last_float": 0, "single_shift_past_end": -1,
    "row_at_int64_max": -1, "row_sum_overflows": -1, "huge_curves_row_at_end": 0, "huge_curves_row_past_end": -1,
    "huge_curves_int32_max_shifts": 0, "weight_nan": -1, "weight_inf": -1, "weight_neg_inf": -1, "weight_negative": -1,
    "weight_neg_zero": 0, "weight_large": 0}


def test_stage_joint_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = dict(l.split() for l in lines[:len(EXPECTED_RC)])
    assert {k: int(v) for k, v in got.items()} == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    # two tables and two key arrays, each padded to 256 bytes; nothing for counts that make no call
    assert rest[0] == "bytes 1024 1024 %d 0 0 0" % (768 + 1024 + 256 + 512)
    # three groups of 93, 1 and 499 shifts: one item of 512 each
    assert rest[1] == ("facts_good rc=0 per=2 items=3 joint=593 grid=3 bytes=1024 g0=(0,0,0,2,93) g1=(1,93,2,1,1) g2=(2,94,3,3,499) "
                       "rows_ok=1 keys_ok=1")
    # 2048 items of 2048 shifts: from there on the large items are taken; one shift row fewer: four times the items of 512
    assert rest[2].startswith("facts_large_items rc=0 per=8 items=2048 joint=4194304 grid=2048 ")
    assert rest[3].startswith("facts_small_items rc=0 per=2 items=8188 joint=4192256 grid=2048 ")
    assert rest[4].startswith("facts_int32_max rc=0 per=8 items=1048576 joint=2147483647 grid=2048 ")
    assert all(l.endswith("rows_ok=1 keys_ok=1") for l in rest[1:5]) and len(rest) == 5


def _run_check(check, tmp_path, method, curves, rows, groups):
    rt = np.array(rows, dtype=_native.JOINT_ROW_DTYPE)
    gt = np.array([(f, m, n, 0) for f, m, n in groups], dtype=_native.JOINT_GROUP_DTYPE)
    paths = [os.path.join(str(tmp_path), name) for name in ("curves", "rows", "groups", "out")]
    for p, a in zip(paths, (curves, rt, gt)):
        a.tofile(p)
    subprocess.check_call([check, "reduce", method.split("_")[0]] + paths)
    raw = np.fromfile(paths[3], np.uint32)
    n_g, n_r = len(groups), len(rows)
    cuts = np.cumsum([0, n_g, n_g, n_r, n_r, n_r])
    idx, score, row_score, row_idx, row_best = (raw[a:b] for a, b in zip(cuts[:-1], cuts[1:]))
    return idx.view(np.int32), score, row_score, row_idx.view(np.int32), row_best, raw[cuts[-1]:]


def _compare_with_joint_host(got, curves, rows, groups, method):
    idx, score, row_score, row_idx, row_best, joint_rows = got
    at = 0
    for g, (first, m, n) in enumerate(groups):
        want = joint.joint_host([curves[o:o + n] for o, _w in rows[first:first + m]], [w for _o, w in rows[first:first + m]], method)
        assert idx[g] == want.index and score[g] == _bits(want.score), (g, m, n)
        assert (row_score[first:first + m] == _bits(want.row_scores)).all(), (g, m, n)
        assert (row_idx[first:first + m] == want.row_own_index).all(), (g, m, n)
        assert (row_best[first:first + m] == _bits(want.row_own_scores)).all(), (g, m, n)
        assert (joint_rows[at:at + n] == _bits(want.joint)).all(), (g, m, n)
        at += n
    assert at == joint_rows.shape[0]


@pytest.mark.parametrize("method", METHODS)
def test_the_header_on_the_cpu_equals_joint_host(check, tmp_path, method):
    """joint_value and the first-extremum rule of joint_core.hpp, run by a program of its own over the ragged groups of the GPU
    test (ties across an item boundary and in the last element, an all-ones group, weights 1/m, 1/3 and 0, odd offsets)."""
    curves, rows, groups = cases.ragged_groups(method, seed=3)
    got = _run_check(check, tmp_path, method, curves, rows, groups)
    _compare_with_joint_host(got, curves, rows, groups, method)
    by_shape = {(m, n): g for g, (_f, m, n) in enumerate(groups)}
    assert got[0][by_shape[(33, 1023)]] == 511 and got[0][by_shape[(3, 4097)]] == 4095 and got[0][by_shape[(9, 65)]] == 0


def test_the_header_on_the_cpu_on_cases_written_here(check, tmp_path):
    # the order-dependent sum, the sum a fused multiply-add would change, signed zeros under ccoeff, one row of one value
    big = np.float32(2.0 ** 60)
    curves = np.array([1, 1, 3, 1, big, big, -big, -big, -1, -1, 3, 3, -0.0, 0.0, 0.0, -0.0, 5], np.float32)
    rows = [(0, 1.0), (2, 1.0), (4, 1.0), (6, 1.0), (8, 1.0), (10, 1.0 / 3.0), (12, 0.5), (14, 0.5), (16, 1.0 / 3.0)]
    groups = [(0, 4, 2), (4, 2, 2), (6, 2, 2), (8, 1, 1)]
    for method in METHODS:
        got = _run_check(check, tmp_path, method, curves, rows, groups)
        _compare_with_joint_host(got, curves, rows, groups, method)
    assert got[0].tolist() == [0, 0, 0, 0] and got[4][6:8].tolist() == [0x80000000, 0]
    assert got[5][:6].tolist() == [0, 0, 0, 0, 0, 0]                    # the swallowed ones; (1/3) * 3 - 1 without a fused multiply-add


# ---------------------------------------------------------------------------------------------- joint_window
def test_joint_window():
    total, W = 100000, 3000
    # interior events: the whole +-W
    assert joint.joint_window([20000, 50000, 70000], [500, 900, 100], total, W) == (-W, 2 * W + 1)
    # an event at the stream's start cuts the low end, one at its end the high end
    assert joint.joint_window([1000, 50000], [500, 900], total, W) == (-1000, 1000 + W + 1)
    assert joint.joint_window([0, 50000], [500, 900], total, W) == (0, W + 1)
    assert joint.joint_window([20000, 99000], [500, 900], total, W) == (-W, W + 100 + 1)
    assert joint.joint_window([20000, 99100], [500, 900], total, W) == (-W, W + 1)
    assert joint.joint_window([700, 99000], [500, 900], total, W) == (-700, 700 + 100 + 1)
    # W = 0: the events where they are
    assert joint.joint_window([20000, 50000], [500, 900], total, 0) == (0, 1)
    assert joint.joint_window([0, total - 900], [500, 900], total, 0) == (0, 1)
    # no displacement serves both: one event would start before the stream, the other end behind it
    for bases, lens in (([-10, 99200], [500, 900]), ([20000, 99101], [500, 900]), ([-1, 50000], [500, 900])):
        with pytest.raises(SushiError):
            joint.joint_window(bases, lens, total, 0 if bases[0] != -10 else W)
    with pytest.raises(SushiError):
        joint.joint_window([], [], total, W)
    with pytest.raises(SushiError):
        joint.joint_window([5], [5, 6], total, W)


# ---------------------------------------------------------------------------------------------- the entry points, no GPU
def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    assert {"sushi_hip_joint_bytes", "sushi_hip_joint_reduce"} <= set(_native.declared_symbols())
    assert L.sushi_hip_joint_bytes(1, 1) == 1024 and L.sushi_hip_joint_bytes(17, 40) == 2560
    assert L.sushi_hip_joint_bytes(0, 5) == 0 and L.sushi_hip_joint_bytes(2, 1) == 0 and L.sushi_hip_joint_bytes(-1, -1) == 0
    rows = np.array([(0, 0.5), (7, 0.5), (100, 1.0)], dtype=_native.JOINT_ROW_DTYPE)
    groups = np.array([(0, 2, 93, 0), (2, 1, 1, 0)], dtype=_native.JOINT_GROUP_DTYPE)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first

    def call(curves=P, n_curve=1000, rows=rows, n_rows=3, groups=groups, n_groups=2, method=0, mem=P, mem_bytes=1 << 16,
             outs=(P, P, P, P, P), joint_out=None):
        return L.sushi_hip_joint_reduce(curves, n_curve, None if rows is None else rows.ctypes.data, n_rows,
                                        None if groups is None else groups.ctypes.data, n_groups, method, mem, mem_bytes,
                                        *outs, joint_out, None)

    EINVAL, EALIGN = -1, -2
    assert call(curves=None) == EINVAL and call(rows=None) == EINVAL and call(groups=None) == EINVAL and call(mem=None) == EINVAL
    for k in range(5):
        assert call(outs=tuple(None if i == k else P for i in range(5))) == EINVAL
    assert call(method=2) == EINVAL and call(method=-1) == EINVAL
    assert call(n_groups=0) == EINVAL and call(n_rows=0) == EINVAL and call(n_rows=1) == EINVAL and call(n_curve=0) == EINVAL
    assert call(n_rows=2) == EINVAL                                     # the groups do not end at n_rows
    for field, at, value in (("first_row", 1, 1), ("n_rows", 0, 0), ("n_rows", 1, 2), ("n_shift", 0, 0), ("n_shift", 0, 994)):
        bad = groups.copy()
        bad[field][at] = value
        assert call(groups=bad) == EINVAL, (field, at, value)
    for field, at, value in (("curve_off", 0, -1), ("curve_off", 1, 908), ("curve_off", 2, 1000), ("curve_off", 2, 2 ** 63 - 1),
                             ("weight", 0, np.nan), ("weight", 1, np.inf), ("weight", 2, -1.0)):
        bad = rows.copy()
        bad[field][at] = value
        assert call(rows=bad) == EINVAL, (field, at, value)
    huge = rows.copy()
    huge["curve_off"][2] = 2 ** 63 - 2
    assert call(rows=huge, n_curve=2 ** 63 - 1, mem_bytes=16) == _native.ENOSPACE    # valid at int64's end; the workspace is what fails
    assert call(mem=ctypes.c_void_p((1 << 20) + 128)) == EALIGN
    assert call(curves=ctypes.c_void_p((1 << 20) + 2)) == EALIGN
    assert call(joint_out=ctypes.c_void_p((1 << 20) + 1)) == EALIGN
    assert call(outs=(P, ctypes.c_void_p((1 << 20) + 2), P, P, P)) == EALIGN
    assert call(mem_bytes=1023) == _native.ENOSPACE and call(mem_bytes=0) == _native.ENOSPACE


def test_joint_tables_are_checked_in_python():
    for rows, groups in (([(0, 1.0)], [(0, 1, 11)]), ([(0, 1.0), (0, 1.0)], [(0, 1, 5)]), ([(0, 1.0)], [(1, 1, 5)]),
                         ([(-1, 1.0)], [(0, 1, 5)]), ([(0, -1.0)], [(0, 1, 5)]), ([(0, 1.0)], [(0, 1, 0)]), ([], [])):
        with pytest.raises(SushiError):
            joint._tables(rows, groups, 10)
    rt, gt = joint._tables([(0, 0.5), (5, 0.5)], [(0, 2, 5)], 10)
    assert rt.dtype == _native.JOINT_ROW_DTYPE and gt.dtype == _native.JOINT_GROUP_DTYPE and gt["n_shift"].tolist() == [5]


# ---------------------------------------------------------------------------------------------- the decoy scenario on the oracle
def test_a_group_finds_what_a_lone_search_misses(oracle):
    """The oracle alone shows both facts: the victim's lone arg-min is the decoy, the arg-min of the five rows' sum the true shift."""
    dst, src = cases.decoy_streams()
    patterns = [src.get_substream(s, e) for s, e in cases.EVENTS]
    bases = [dst._get_sample_for_time(s) for s, _e in cases.EVENTS]
    k_lo, n_shift = joint.joint_window(bases, [p.shape[1] for p in patterns], dst.data.shape[1], int(cases.RATE * cases.WINDOW))
    assert (k_lo, n_shift) == (cases.K_LO, cases.N_SHIFT)
    rows = cases.oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift)
    lone = [oracle.argmin_first(r) + k_lo for r in rows]
    assert lone == cases.LONE_K and lone[cases.VICTIM] == cases.OFFSET + cases.DECOY
    assert int(_bits(rows[cases.VICTIM].min())[0]) == cases.VICTIM_LONE_SCORE_BITS
    got = joint.joint_host(rows, [1.0 / 5] * 5)
    assert got.index + k_lo == cases.JOINT_K == cases.OFFSET
    assert int(_bits(got.score)[0]) == cases.JOINT_SCORE_BITS and _bits(got.row_scores).tolist() == cases.EVENT_SCORE_BITS
    assert (got.row_own_index + k_lo).tolist() == cases.LONE_K
    # the victim's own score at the true shift is worse than at the decoy: alone it cannot tell
    assert got.row_scores[cases.VICTIM] > got.row_own_scores[cases.VICTIM]
