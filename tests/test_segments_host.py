"""Segmentation without a GPU: the NumPy restatement of sushi_hip_path_forward / sushi_hip_path_backtrack (sushi_amd/segments.py
path_host) against the loop written out and against a brute force over all paths, planted ties, penalty extremes, the kernels' own
header compiled for the CPU (tests/host_path_check.cpp, a program of its own under AddressSanitizer + UBSan), the entry points'
argument checks, and the two-cut scenario on the CPU oracle."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

import segment_cases as cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, axis, joint, segments
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("path_check")), "host_path_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_path_check.cpp"), "-o", exe])
    return exe


def _loop(rows, weights, lam, method):
    """The definition, written out: one shift at a time on Python floats (IEEE float64).  -> (shifts, cost, row_min, row_arg)"""
    E, n = len(rows), rows[0].shape[0]
    sign = -1.0 if method == "ccoeff_normed" else 1.0
    D, stay, row_min, row_arg = None, [None] * E, [], []
    for e in range(E):
        u = [float(weights[e]) * (-float(rows[e][j]) if sign < 0 else float(rows[e][j])) for j in range(n)]
        if e == 0:
            D = u
        else:
            jump = row_min[e - 1] + lam
            stay[e] = [D[j] <= jump for j in range(n)]
            D = [u[j] + (D[j] if stay[e][j] else jump) for j in range(n)]
        at = 0
        for j in range(1, n):
            if D[j] < D[at]:
                at = j
        row_arg.append(at)
        row_min.append(D[at])
    s = row_arg[-1]
    shifts = [s]
    for e in range(E - 1, 0, -1):
        if not stay[e][s]:
            s = row_arg[e - 1]
        shifts.append(s)
    return shifts[::-1], row_min[-1], row_min, row_arg


def _first(row, method):
    at = 0
    for j in range(1, row.shape[0]):
        if (row[j] > row[at]) if method == "ccoeff_normed" else (row[j] < row[at]):
            at = j
    return at


def _rows(E, n, seed, method="sqdiff_normed"):
    rng = np.random.default_rng(seed)
    lo = 0.0 if method == "sqdiff_normed" else -1.0
    return [(rng.random(n, dtype=np.float32) * np.float32(1.0 - lo) + np.float32(lo)).astype(np.float32) for _ in range(E)]


def _path_cost(rows, weights, lam, method, path):
    """A path's cost accumulated in the pass's order: c = u_0[s_0]; per event c = c + lam if the shift changed, then c + u_e[s_e]."""
    u = lambda e: float(weights[e]) * (-float(rows[e][path[e]]) if method == "ccoeff_normed" else float(rows[e][path[e]]))
    c = u(0)
    for e in range(1, len(rows)):
        if path[e] != path[e - 1]:
            c = c + lam
        c = c + u(e)
    return c


# ---------------------------------------------------------------------------------------------- path_host
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("E", [1, 2, 7, 33])
@pytest.mark.parametrize("n", [1, 63, 65, 1025])
def test_path_host_is_the_loop_written_out(E, n, method):
    rows = _rows(E, n, seed=E * 10007 + n, method=method)
    for weights, lam in (([1.0] * E, 0.25), ([(1.0 / 3.0, 0.0, 2.5)[i % 3] for i in range(E)], 1.0 / 3.0), ([1.0] * E, 0.0)):
        got = segments.path_host(rows, weights, lam, method)
        shifts, cost, row_min, row_arg = _loop(rows, weights, lam, method)
        assert got.shifts.tolist() == shifts and got.row_arg.tolist() == row_arg
        assert (_bits64(got.row_min) == _bits64(row_min)).all() and _bits64(got.cost) == _bits64(cost)
        own = [_first(r, method) for r in rows]
        assert got.row_own_index.tolist() == own
        assert (_bits(got.row_own_scores) == _bits([r[k] for r, k in zip(rows, own)])).all()
        assert got.shifts.dtype == np.int32 and got.row_arg.dtype == np.int32 and got.row_min.dtype == np.float64


@pytest.mark.parametrize("method", METHODS)
def test_the_pass_finds_the_minimum_over_all_paths(method):
    """E <= 5, n_shift <= 4, dyadic values (every sum exact, so ties are real ties): path_host's cost is the minimum over all
    n_shift^E paths of the in-order cost, exactly, and its own path attains it."""
    rng = np.random.default_rng(5)
    sign = -1.0 if method == "ccoeff_normed" else 1.0
    for E, n in itertools.product((1, 2, 3, 5), (1, 2, 3, 4)):
        for trial in range(6):
            rows = [(sign * rng.integers(0, 17, n) / 16.0).astype(np.float32) for _ in range(E)]
            weights = [(1.0, 0.5, 2.0, 0.0)[int(k)] for k in rng.integers(0, 4, E)]
            lam = (0.0, 0.125, 0.5, 1.0, 4.0, 0.3)[trial]
            got = segments.path_host(rows, weights, lam, method)
            costs = [_path_cost(rows, weights, lam, method, p) for p in itertools.product(range(n), repeat=E)]
            assert got.cost == min(costs), (E, n, trial)
            assert _path_cost(rows, weights, lam, method, got.shifts.tolist()) == got.cost, (E, n, trial)


def test_a_tie_between_staying_and_jumping_stays():
    # D_0 = [0.75, 0.25]: m_0 = 0.25 at 1, jump_1 = 0.75 = D_0[0] exactly: index 0 stays; D_1 = [1.0, 1.0]: the first index wins
    rows = [np.array([0.75, 0.25], np.float32), np.array([0.25, 0.75], np.float32)]
    got = segments.path_host(rows, [1.0, 1.0], 0.5)
    assert got.row_arg.tolist() == [1, 0] and got.row_min.tolist() == [0.25, 1.0]
    assert got.shifts.tolist() == [0, 0] and got.cost == 1.0          # (a jump would have come from index 1: the same cost)
    # the issue's rows: nothing to gain from a change
    same = segments.path_host([np.array([0.25, 0.75], np.float32)] * 2, [1.0, 1.0], 0.5)
    assert same.shifts.tolist() == [0, 0] and same.cost == 0.5 and same.row_min.tolist() == [0.25, 0.5]
    # one ulp above the tie jumps
    up = np.nextafter(np.float32(0.75), np.float32(1.0))
    got = segments.path_host([np.array([up, 0.25], np.float32), np.array([0.25, 0.75], np.float32)], [1.0, 1.0], 0.5)
    assert got.shifts.tolist() == [1, 0] and got.cost == 1.0


@pytest.mark.parametrize("method", METHODS)
def test_equal_minima_take_the_first_index(method):
    best = np.float32(0.0 if method == "sqdiff_normed" else 1.0)
    rows = _rows(3, 65, seed=9, method=method)
    rows = [np.clip(r, np.float32(0.01), np.float32(0.99)) if method == "sqdiff_normed" else np.clip(r, np.float32(-0.9), np.float32(0.9))
            for r in rows]
    for r in rows:
        r[[20, 41, 64]] = best
    got = segments.path_host(rows, [1.0] * 3, 0.5, method)
    assert got.shifts.tolist() == [20] * 3 and got.row_arg.tolist() == [20] * 3 and got.row_own_index.tolist() == [20] * 3
    flat = segments.path_host([np.ones(63, np.float32)] * 4, [1.0] * 4, 0.5, method)
    assert flat.shifts.tolist() == [0] * 4 and flat.cost == (4.0 if method == "sqdiff_normed" else -4.0)


def test_signed_zeros_tie_under_ccoeff():
    """0.0 and -0.0 compare equal: the first of them is the extremum, and a row's own value is returned with its own bits."""
    a = np.array([-0.5, -0.0, 0.0, -0.0], np.float32)
    b = np.array([-0.5, 0.0, -0.0, 0.0], np.float32)
    got = segments.path_host([a, b], [1.0, 1.0], 0.5, "ccoeff_normed")
    assert got.shifts.tolist() == [1, 1] and got.row_arg.tolist() == [1, 1] and got.row_own_index.tolist() == [1, 1]
    assert _bits(got.row_own_scores).tolist() == [0x80000000, 0x00000000]
    # c = -R: D_0[1] = 1.0 * -(-0.0) = 0.0; D_1[1] = -0.0 + 0.0 = 0.0
    assert _bits64(got.row_min).tolist() == [0, 0]
    shifts, cost, row_min, row_arg = _loop([a, b], [1.0, 1.0], 0.5, "ccoeff_normed")
    assert (shifts, row_arg) == ([1, 1], [1, 1]) and _bits64(row_min).tolist() == [0, 0]


def test_a_row_of_weight_zero_follows_its_neighbours():
    rows = _rows(3, 33, seed=4)
    for r in rows:
        r[:] = np.clip(r, np.float32(0.2), None)
    rows[0][5] = rows[2][5] = np.float32(0.0625)
    rows[1][20] = np.float32(0.0)                       # the middle row's own best is elsewhere, and counts for nothing
    got = segments.path_host(rows, [1.0, 0.0, 1.0], 0.25)
    assert got.shifts.tolist() == [5, 5, 5] and got.cost == 0.125 and got.row_own_index.tolist() == [5, 20, 5]
    # every D of the weightless row is the row before it, capped: its first minimum is the one before
    assert got.row_arg.tolist() == [5, 5, 5] and got.row_min.tolist() == [0.0625, 0.0625, 0.125]


@pytest.mark.parametrize("method", METHODS)
def test_penalty_extremes(method):
    E, n = 9, 257
    rows = _rows(E, n, seed=77, method=method)            # (tie-free: 257 random float32 values a row)
    assert all(np.unique(r).shape[0] == n for r in rows)
    weights = [1.0, 0.5, 2.0] * 3
    own = [_first(r, method) for r in rows]
    free = segments.path_host(rows, weights, 0.0, method)
    assert free.shifts.tolist() == own == free.row_own_index.tolist()
    # a huge finite penalty: one segment, at the arg-min of the in-order float64 sum
    total = [0.0] * n
    for e in range(E):
        for j in range(n):
            u = weights[e] * (-float(rows[e][j]) if method == "ccoeff_normed" else float(rows[e][j]))
            total[j] = u if e == 0 else total[j] + u
    at = min(range(n), key=lambda j: (total[j], j))
    rigid = segments.path_host(rows, weights, 1e30, method)
    assert rigid.shifts.tolist() == [at] * E and _bits64(rigid.cost) == _bits64(total[at])
    assert segments.runs(rigid.shifts.tolist()) == [(0, E, at)]


def test_path_host_refuses_bad_arguments():
    r = np.zeros(4, np.float32)
    for rows, weights in (([], []), ([r], [1.0, 1.0]), ([r, np.zeros(5, np.float32)], [1, 1]), ([r.astype(np.float64)], [1.0]),
                          ([np.zeros(0, np.float32)], [1.0]), ([r], [-1.0]), ([r], [float("nan")]), ([r], [float("inf")]),
                          ([r.reshape(1, 4)], [1.0])):
        with pytest.raises(SushiError):
            segments.path_host(rows, weights, 0.5)
    for lam in (-0.5, float("nan"), float("inf"), "much", None):
        with pytest.raises(SushiError):
            segments.path_host([r], [1.0], lam)
    with pytest.raises(SushiError):
        segments.path_host([r], [1.0], 0.5, "sqdiff")


def test_runs():
    assert segments.runs([]) == [] and segments.runs([4]) == [(0, 1, 4)]
    assert segments.runs([3, 3, -1, -1, -1, 3]) == [(0, 2, 3), (2, 3, -1), (5, 1, 3)]


# ---------------------------------------------------------------------------------------------- the kernels' header on the CPU
EXPECTED_RC = {   # case of host_path_check validate -> what stage_path returns
    "good": 0, "good_ccoeff": 0, "null_rows": -1, "null_mem": -1, "method_2": -1, "method_neg": -1, "no_rows": -1, "negative_rows": -1,
    "no_shift": -1, "negative_shift": -1, "empty_curves": -1, "negative_curves": -1, "shift_beyond_curves": -1,
    "whole_sequence": 0, "rows_end_at_sequence_end": 0, "rows_past_sequence_end": -1, "row0_negative": -1, "row0_at_end": -1,
    "no_total": -1, "negative_total": -1, "rows_end_at_int_max": 0, "rows_sum_overflows_int": -1, "row0_int_max": -1,
    "row_before_curves": -1, "row_ends_at_curves_end": 0, "row_one_past_curves_end": -1, "single_shift_last_float": 0,
    "single_shift_past_end": -1, "row_at_int64_max": -1, "row_sum_overflows": -1, "huge_curves_row_at_end": 0,
    "huge_curves_row_past_end": -1, "huge_curves_int32_max_shifts": 0, "weight_nan": -1, "weight_inf": -1, "weight_neg_inf": -1,
    "weight_negative": -1, "weight_neg_zero": 0, "weight_large": 0, "penalty_nan": -1, "penalty_inf": -1, "penalty_negative": -1,
    "penalty_zero": 0, "penalty_neg_zero": 0, "penalty_large": 0, "workspace_exact": 0, "workspace_short": -4, "workspace_none": -4,
    "workspace_misaligned": -2, "workspace_misaligned_and_short": -2, "bad_tables_before_workspace": -1}


def test_stage_path_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = dict(l.split() for l in lines[:len(EXPECTED_RC)])
    assert {k: int(v) for k, v in got.items()} == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    # two sets of one record of 20 bytes per workgroup, each set padded to 256 bytes; nothing for counts that make no call
    assert rest[0] == "bytes 512 512 %d %d 0 0 0" % (2 * 9472, 2 * 40960)
    assert rest[1] == "words 1 1 2 33554432 0 0"
    assert rest[2] == "facts_one rc=0 per=2 items=1 grid=1 words=1 set=256 bytes=512 offsets=(0,8,12,16)"
    assert rest[3] == "facts_512 rc=0 per=2 items=1 grid=1 words=8 set=256 bytes=512 offsets=(0,8,12,16)"
    assert rest[4] == "facts_513 rc=0 per=2 items=2 grid=2 words=9 set=256 bytes=512 offsets=(0,16,24,32)"
    assert rest[5] == "facts_240001 rc=0 per=2 items=469 grid=469 words=3751 set=9472 bytes=18944 offsets=(0,3752,5628,7504)"
    # 1024 items of 2048 shifts: from there on the large items are taken; one shift fewer: four times the items of 512
    assert rest[6].startswith("facts_large_items rc=0 per=8 items=1024 grid=1024 words=32737 ")
    assert rest[7].startswith("facts_small_items rc=0 per=2 items=4092 grid=2048 words=32736 ")
    assert rest[8].startswith("facts_2880001 rc=0 per=8 items=1407 grid=1407 words=45001 ")
    assert rest[9].startswith("facts_int32_max rc=0 per=8 items=1048576 grid=2048 words=33554432 set=40960 bytes=81920 ")
    assert len(rest) == 10 and cases.PER_LARGE_FROM == 1023 * 2048 + 1


def _run_check(check, tmp_path, method, lam, n, curves, rows):
    rt = np.array(rows, dtype=_native.JOINT_ROW_DTYPE)
    paths = [os.path.join(str(tmp_path), name) for name in ("curves", "rows", "out")]
    curves.tofile(paths[0])
    rt.tofile(paths[1])
    subprocess.check_call([check, "pass", method.split("_")[0], float(lam).hex(), str(n)] + paths)
    raw = np.fromfile(paths[2], np.uint8)
    E = len(rows)
    shifts, row_arg, own_idx = (raw[4 * E * k:4 * E * (k + 1)].view(np.int32) for k in range(3))
    own_val = raw[12 * E:16 * E].view(np.uint32)
    row_min = raw[16 * E:24 * E].view(np.uint64)
    return shifts, row_arg, own_idx, own_val, row_min, raw[24 * E:].view(np.uint64)


def _compare_with_path_host(got, rows, weights, lam, method):
    shifts, row_arg, own_idx, own_val, row_min, stay = got
    want = segments.path_host(rows, weights, lam, method)
    assert shifts.tolist() == want.shifts.tolist() and row_arg.tolist() == want.row_arg.tolist()
    assert own_idx.tolist() == want.row_own_index.tolist() and (own_val == _bits(want.row_own_scores)).all()
    assert (row_min == _bits64(want.row_min)).all()
    assert (stay == cases.stay_words(rows, weights, lam, method).reshape(-1)).all()
    return want


@pytest.mark.parametrize("method", METHODS)
def test_the_header_on_the_cpu_equals_path_host(check, tmp_path, method):
    """path_cost, path_step, both first-extremum rules and path_backtrack of path_core.hpp, run by a program of its own over the
    sequences of the GPU test but the longest (ties across a workgroup boundary and in the last element, an all-ones sequence,
    weights 1, 1/3, 0 and 2.5, odd offsets) -- divided as the kernels divide them, every open order taken backwards."""
    for E, n in cases.SHAPES[:-1] + [(4, 1025)]:
        curves, rows, weights, lam = cases.sequence(E, n, method, seed=3)
        want = _compare_with_path_host(_run_check(check, tmp_path, method, lam, n, curves, rows), cases.rows_of(curves, rows, n),
                                       weights, lam, method)
        if (E, n) == (33, 1023):
            assert want.shifts.tolist() == [511] * 33
        if (E, n) == (3, 4097):
            assert want.shifts.tolist() == [4095] * 3
        if (E, n) == (9, 65):
            assert want.shifts.tolist() == [0] * 9
        if (E, n) == (7, 64):
            assert len(segments.runs(want.shifts.tolist())) > 1            # a sequence whose path does change


def test_the_header_on_the_cpu_on_cases_written_here(check, tmp_path):
    # the exact stay / jump tie; signed zeros under ccoeff; a weightless row; a sum a fused multiply-add would change:
    # u = (1/3) * 3 rounds to 1, and -1 + 1 is 0 where a fused form leaves -2^-54 (which would not tie with the 0.0 beside it)
    curves = np.array([0.75, 0.25, 0.25, 0.75, -0.5, -0.0, 0.0, -0.0, -0.5, 0.0, -0.0, 0.0, 3, 3, 0, 0], np.float32)
    for method in METHODS:
        for rows, n, lam in (([(0, 1.0), (2, 1.0)], 2, 0.5), ([(4, 1.0), (8, 1.0)], 4, 0.5), ([(0, 1.0), (1, 0.0), (2, 1.0)], 2, 0.25),
                             ([(12, 1.0 / 3.0), (14, 1.0)], 2, 0.0)):
            got = _run_check(check, tmp_path, method, lam, n, curves, rows)
            _compare_with_path_host(got, cases.rows_of(curves, rows, n), [w for _o, w in rows], lam, method)
    fma = _run_check(check, tmp_path, "sqdiff_normed", 0.0, 2, np.array([-1, 0, 3, 3], np.float32), [(0, 1.0), (2, 1.0 / 3.0)])
    assert fma[0].tolist() == [0, 0] and fma[4].tolist() == _bits64([-1.0, 0.0]).tolist()


# ---------------------------------------------------------------------------------------------- the entry points, no GPU
def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    assert {"sushi_hip_path_bytes", "sushi_hip_path_stay_words", "sushi_hip_path_forward", "sushi_hip_path_backtrack"} <= \
        set(_native.declared_symbols())
    assert L.sushi_hip_path_bytes(1, 1) == 512 and L.sushi_hip_path_bytes(200, 240001) == 18944
    assert L.sushi_hip_path_bytes(0, 5) == 0 and L.sushi_hip_path_bytes(5, 0) == 0 and L.sushi_hip_path_bytes(-1, -1) == 0
    assert [L.sushi_hip_path_stay_words(n) for n in (1, 64, 65, 240001, 0, -4)] == [1, 1, 2, 3751, 0, 0]
    rows = np.array([(0, 1.0), (501, 0.0), (333, 2.5)], dtype=_native.JOINT_ROW_DTYPE)
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first
    odd = lambda k: ctypes.c_void_p((1 << 20) + k)

    def call(curves=P, n_curve=1000, rows=rows, n_rows=3, n_shift=499, method=0, penalty=0.5, row0=2, n_total=7,
             outs=(P, P, P, P, P, P), mem=P, mem_bytes=1 << 16):
        return L.sushi_hip_path_forward(curves, n_curve, None if rows is None else rows.ctypes.data, n_rows, n_shift, method, penalty,
                                        row0, n_total, *outs, mem, mem_bytes, None)

    EINVAL, EALIGN = -1, -2
    assert call(curves=None) == EINVAL and call(rows=None) == EINVAL and call(mem=None) == EINVAL
    for k in range(6):
        assert call(outs=tuple(None if i == k else P for i in range(6))) == EINVAL
    assert call(method=2) == EINVAL and call(method=-1) == EINVAL
    assert call(n_rows=0) == EINVAL and call(n_shift=0) == EINVAL and call(n_curve=0) == EINVAL and call(n_shift=1001) == EINVAL
    assert call(row0=-1) == EINVAL and call(row0=5) == EINVAL and call(n_total=0) == EINVAL and call(row0=7) == EINVAL
    assert call(row0=2 ** 31 - 3, n_total=2 ** 31 - 1) == EINVAL          # row0 + n_rows would pass int: never formed
    for lam in (np.nan, np.inf, -1e-300):
        assert call(penalty=lam) == EINVAL
    for field, at, value in (("curve_off", 0, -1), ("curve_off", 1, 502), ("curve_off", 2, 2 ** 63 - 1), ("weight", 0, np.nan),
                             ("weight", 1, np.inf), ("weight", 2, -1.0)):
        bad = rows.copy()
        bad[field][at] = value
        assert call(rows=bad) == EINVAL, (field, at, value)
    huge = rows.copy()
    huge["curve_off"][2] = 2 ** 63 - 500
    assert call(rows=huge, n_curve=2 ** 63 - 1, mem_bytes=16) == _native.ENOSPACE    # valid at int64's end; the workspace is what fails
    assert call(mem=odd(128)) == EALIGN and call(mem_bytes=511) == _native.ENOSPACE and call(mem_bytes=0) == _native.ENOSPACE
    assert call(curves=odd(2)) == EALIGN
    for k, off in enumerate((4, 4, 4, 2, 2, 2)):      # D, stay, row_min: 8 bytes; row_arg, row_own_index, row_own_score: 4
        assert call(outs=tuple(odd(off) if i == k else P for i in range(6))) == EALIGN, k

    def back(stay=P, row_arg=P, n_total=7, n_shift=499, out=P):
        return L.sushi_hip_path_backtrack(stay, row_arg, n_total, n_shift, out, None)

    assert back(stay=None) == EINVAL and back(row_arg=None) == EINVAL and back(out=None) == EINVAL
    assert back(n_total=0) == EINVAL and back(n_shift=0) == EINVAL and back(n_total=-1) == EINVAL
    assert back(stay=odd(4)) == EALIGN and back(row_arg=odd(2)) == EALIGN and back(out=odd(2)) == EALIGN


class _NoDevice(object):
    """A stream that fails the moment find_segments asks it for device memory: every check in front of that is host work."""
    sample_rate = 12000
    data = np.zeros((1, 400000), np.uint8)

    def device_stream(self):
        return None

    def _pattern_source(self, patterns, dst_dev):
        return None, [0] * len(patterns), [p.shape[1] for p in patterns], True

    def _get_sample_for_time(self, t):
        return int(self.sample_rate * t) + 120000


def test_find_segments_names_the_state_it_cannot_hold():
    stream = _NoDevice()
    patterns = [np.zeros((1, 6000), np.uint8)] * 4
    centres = [1.0, 2.0, 3.0, 4.0]
    need = 4 * ((24001 + 63) // 64) * 8 + 24001 * 8
    assert segments.PathState.nbytes(4, 24001) == need
    with pytest.raises(SushiError) as e:
        segments.find_segments(stream, patterns, centres, 1.0, 0.5, max_state_bytes=need - 1)
    assert str(need) in str(e.value) and "max_state_bytes" in str(e.value)
    with pytest.raises(SushiError) as e:
        segments.find_segments(stream, patterns, centres, 1.0, 0.5, max_bytes=4 * 24001 - 1)
    assert str(4 * 24001) in str(e.value)
    for bad in dict(penalty=-1.0), dict(penalty=float("nan")), dict(weights="median"), dict(weights=[1.0]), dict(method="sqdiff"):
        kw = dict(penalty=0.5)
        kw.update(bad)
        with pytest.raises(SushiError):
            segments.find_segments(stream, patterns, centres, 1.0, kw.pop("penalty"), **kw)
    with pytest.raises(SushiError):
        segments.find_segments(stream, patterns, centres[:3], 1.0, 0.5)
    with pytest.raises(TypeError):
        segments.find_segments(stream, patterns, centres, 1.0)                # the penalty has no default


def test_weights_are_per_event():
    assert axis.event_weights("equal", [500, 900, 100], per_event=True) == [1.0, 1.0, 1.0]  # not 1 / m: the penalty is per event
    assert axis.event_weights("length", [500, 900, 100], per_event=True) == [1.0, 1.8, 0.2]
    assert axis.event_weights([2, 0, 1], [5, 5, 5], per_event=True) == [2.0, 0.0, 1.0]


# ---------------------------------------------------------------------------------------------- the two-cut scenario on the oracle
@pytest.fixture(scope="module")
def oracle_case(oracle):
    dst, src = cases.two_cut_streams()
    patterns, _centres, bases = cases.scenario(dst, src)
    k_lo, n_shift = joint.joint_window(bases, [p.shape[1] for p in patterns], dst.data.shape[1], int(cases.RATE * cases.WINDOW))
    return k_lo, n_shift, cases.oracle_rows(oracle, dst, patterns, bases, k_lo, n_shift)


def test_the_pass_finds_the_cut_neither_search_finds(oracle, oracle_case):
    """The oracle alone shows all three facts: lone searches place both victims at their decoys, one joint search over all ten
    events places the first half at the second half's shift, and the pass returns the two segments -- for every penalty from 0.1
    to 2.0."""
    k_lo, n_shift, rows = oracle_case
    assert (k_lo, n_shift) == (cases.K_LO, cases.N_SHIFT)
    lone = [oracle.argmin_first(r) + k_lo for r in rows]
    assert lone == cases.LONE_K
    for v, d in zip(cases.VICTIMS, cases.DECOYS):
        assert lone[v] == cases.TRUE_K[v] + d
    whole = joint.joint_host(rows, [0.1] * 10)
    assert whole.index + k_lo == cases.JOINT_K
    for e in range(5):                                  # the first half at the joint answer, against its own shift (two decimals)
        assert 0.44 <= round(float(rows[e][whole.index]), 2) <= 0.69
        assert 0.12 <= round(float(rows[e][cases.TRUE_K[e] - k_lo]), 2) <= 0.20
    for lam in cases.PENALTIES_THAT_FIND_THE_CUT:
        got = segments.path_host(rows, [1.0] * 10, lam)
        assert (got.shifts + k_lo).tolist() == cases.TRUE_K, lam
        assert segments.runs((got.shifts + k_lo).tolist()) == [(0, 5, 3000), (5, 5, -2400)]
    got = segments.path_host(rows, [1.0] * 10, cases.PENALTY)
    assert got.cost == cases.COST
    assert _bits([r[s] for r, s in zip(rows, got.shifts)]).tolist() == cases.EVENT_SCORE_BITS
    assert (got.row_own_index + k_lo).tolist() == cases.LONE_K and _bits(got.row_own_scores).tolist() == cases.OWN_SCORE_BITS


def test_the_penalty_extremes_of_the_scenario(oracle_case):
    k_lo, _n, rows = oracle_case
    for lam, shifts, cost in cases.EXTREMES:
        got = segments.path_host(rows, [1.0] * 10, lam)
        assert (got.shifts + k_lo).tolist() == shifts and got.cost == cost, lam
