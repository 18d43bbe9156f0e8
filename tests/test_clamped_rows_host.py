"""Clamped score rows without a GPU: the rule (sushi_amd/axis.py clamp_value, clamp_rows_host) against loops written out here, the
kernels' own header compiled for the CPU (tests/host_rows_check.cpp, a program of its own under AddressSanitizer + UBSan) against
the NumPy restatement (sushi_amd/rows.py rows_from_hits_host) over hit lists at tile edges, the entry points' argument checks, the
clamp= / capacity= checks of the four searches, and the stream scenario's hit counts on the CPU oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import clamped_rows_cases as cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, axis, rows
from sushi_amd.common import SushiError

METHODS = ("sqdiff_normed", "ccoeff_normed")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _b(x):
    return int(np.float32(x).view(np.uint32))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("rows_check")), "host_rows_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_rows_check.cpp"), "-o", exe])
    return exe


# ---------------------------------------------------------------------------------------------- clamp_value
def test_clamp_value_rounds_towards_the_side_that_fails():
    below, above = np.float32(0.7), np.nextafter(np.float32(0.7), np.float32(1.0))
    assert float(below) < 0.7 < float(above)                        # 0.7 lies between two float32s; the nearest is the lower one
    assert _bits(axis.clamp_value(0.7, "sqdiff_normed")) == _bits(above)
    assert _bits(axis.clamp_value(0.7, "ccoeff_normed")) == _bits(below)
    up = np.float32(0.6)
    assert float(up) > 0.6                                          # ... and here the nearest is the upper one
    assert _bits(axis.clamp_value(0.6, "sqdiff_normed")) == _bits(up)
    assert _bits(axis.clamp_value(0.6, "ccoeff_normed")) == _bits(np.nextafter(up, np.float32(0.0)))
    for method in METHODS:
        for exact in (0.5, 0.0, -0.25, 3.0, float(above), np.float32(0.1)):
            f = axis.clamp_value(exact, method)
            assert f.dtype == np.float32 and float(f) == float(exact)
        for c in (0.6, 0.7, 0.3, -0.7, 1e-50, -1e-50, 1.0 / 3.0):
            f = axis.clamp_value(c, method)
            # the float32 on the failing side, and the nearest such: the next one towards clamp is on the other side of it
            if method == "sqdiff_normed":
                assert float(f) >= c and float(np.nextafter(f, np.float32(-np.inf))) < c
            else:
                assert float(f) <= c and float(np.nextafter(f, np.float32(np.inf))) > c
    assert _bits(axis.clamp_value(-0.0, "ccoeff_normed")) == 0x80000000


def test_clamp_value_refuses_what_is_not_a_finite_number():
    for method in METHODS:
        for bad in (float("nan"), float("inf"), float("-inf"), "high", None, 1e39 if method == "sqdiff_normed" else -1e39):
            with pytest.raises(SushiError):
                axis.clamp_value(bad, method)
    with pytest.raises(SushiError):
        axis.clamp_value(0.5, "sqdiff")
    # the largest float32 is still a clamp; a number beyond it only on the side whose float32 is finite
    big = float(np.finfo(np.float32).max)
    assert float(axis.clamp_value(big, "sqdiff_normed")) == big and float(axis.clamp_value(1e39, "ccoeff_normed")) == big
    assert float(axis.clamp_value(-1e39, "sqdiff_normed")) == -big


# ---------------------------------------------------------------------------------------------- clamp_rows_host
def _clamp_loop(row, f, method):
    """The definition, written out: one value at a time, compared as Python floats (IEEE float64)."""
    out = np.empty(row.shape[0], np.float32)
    for j in range(row.shape[0]):
        v = float(row[j])
        keep = (v >= float(f)) if method == "ccoeff_normed" else (v <= float(f))
        out[j] = row[j] if keep else f
    return out


@pytest.mark.parametrize("method", METHODS)
def test_clamp_rows_host_is_the_loop_written_out(method):
    rng = np.random.default_rng(5)
    row = (rng.random(1025, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    for clamp in (0.6, 0.3, -0.2, 0.0):
        f = axis.clamp_value(clamp, method)
        row[[3, 500, 1024]] = f                                     # a value equal to f passes: its own bits, which are f's
        row[[4, 501]] = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
        got = axis.clamp_rows_host(row, clamp, method)
        assert got.dtype == np.float32 and (_bits(got) == _bits(_clamp_loop(row, f, method))).all()
        passing = row >= f if method == "ccoeff_normed" else row <= f
        assert 0 < passing.sum() < row.shape[0] and (_bits(got[passing]) == _bits(row[passing])).all() and (got[~passing] == f).all()
    two = np.stack([row, row[::-1]])
    assert (_bits(axis.clamp_rows_host(two, 0.3, method)[1]) == _bits(axis.clamp_rows_host(row[::-1], 0.3, method))).all()
    with pytest.raises(SushiError):
        axis.clamp_rows_host(row.astype(np.float64), 0.3, method)


@pytest.mark.parametrize("method", METHODS)
def test_signed_zeros_pass_a_clamp_of_zero_with_their_own_bits(method):
    row = np.array([-0.0, 0.0, 0.5, -0.5, np.nan], np.float32)
    got = _bits(axis.clamp_rows_host(row, 0.0, method))
    keep = [0x80000000, 0, 0, _b(-0.5), 0] if method == "sqdiff_normed" else [0x80000000, 0, _b(0.5), 0, 0]
    assert got.tolist() == keep
    got = _bits(axis.clamp_rows_host(row, -0.0, method))            # f = -0.0: what fails becomes -0.0
    assert got[0] == 0x80000000 and got[1] == 0 and got[4] == 0x80000000


# ---------------------------------------------------------------------------------------------- the kernels' header on the CPU
EXPECTED_RC = {
    "good": 0, "good_with_in": 0, "no_rows": -1, "negative_rows": -1, "empty_out": -1, "empty_in": -1, "fill_nan": -1, "fill_inf": -1,
    "fill_neg_zero": 0, "row_empty": -1, "row_negative": -1, "row_before_out": -1, "row_ends_at_out_end": 0, "row_one_past_out_end": -1,
    "row_one_past_in_end": -1, "row_before_in": -1, "in_not_read_without_in": 0, "row_at_int64_max": -1, "huge_out_row_at_end": 0,
    "huge_out_row_past_end": -1, "int32_max_floats": 0}


def test_stage_rows_validation_and_layout(check):
    lines = subprocess.check_output([check, "validate"]).decode().splitlines()
    got = dict(l.split() for l in lines[:len(EXPECTED_RC)])
    assert {k: int(v) for k, v in got.items()} == EXPECTED_RC
    rest = lines[len(EXPECTED_RC):]
    T = cases.T
    assert T == 4096 and rest[0] == "facts_int32_max items=%d grid=2048 tiles=%d" % (2 + 2 ** 31 // T, 2 ** 31 // T)
    # rows of 5, T and 3 T + 5 floats: one, one and four tiles; every item finds its row
    assert rest[1] == "facts_good rc=0 items=6 grid=6 bytes=256 r0=(1,0,0,5,1) r1=(7,3,1,4096,1) r2=(5001,9000,2,12293,4)"
    assert rest[2] == "row_of 0 1 2 2 2 2"
    assert rest[3] == "bytes 256 256 512 0"
    # apart; in place; the same first float with a row moved; one float apart; the last float shared
    assert rest[4] == "overlap 1 1 0 0 0" and len(rest) == 5


def _form(check, tmp_path, call):
    paths = [os.path.join(str(tmp_path), name) for name in ("hits", "counts", "table", "out")]
    for p, a in zip(paths, (call["hits"], call["counts"], call["table"])):
        np.ascontiguousarray(a).tofile(p)
    subprocess.check_call([check, "form", "%08x" % _b(call["f"]), str(call["capacity"]), str(call["n_out"])] + paths)
    raw = np.fromfile(paths[3], np.uint32)
    return raw[:call["n_out"]], raw[call["n_out"]:].view(np.int32)


def _written_out(call, k):
    """Row k of a call whose list is good: f, then every hit's score at its index."""
    n_pos, count = int(call["table"]["n_pos"][k]), int(call["counts"][k])
    row = np.full(n_pos, call["f"], np.float32)
    for j in range(count if count <= call["capacity"] else 0):
        row[call["hits"][k, j, 0]] = call["hits"][k, j:j + 1, 1].view(np.float32)[0]
    return row


def test_the_header_on_the_cpu_equals_the_restatement(check, tmp_path):
    """rows_core.hpp's tile-range search, fill and checks, run tile by tile by a program of its own over the synthetic calls of the
    GPU test: equal to rows_from_hits_host bit for bit, flags included; rows with good lists equal the loop written out; no float
    outside a row is touched."""
    seen = set()
    for call in cases.synthetic_calls():
        got, got_flags = _form(check, tmp_path, call)
        want, want_flags = cases.expected(call)
        assert (got == want.view(np.uint32)).all() and got_flags.tolist() == want_flags.tolist()
        assert (got[cases.outside_rows(call)] == cases.SENTINEL_BITS).all()
        for k, flag in enumerate(want_flags):
            off, n_pos = int(call["table"]["out_off"][k]), int(call["table"]["n_pos"][k])
            if not flag & rows.BAD_HITS:
                assert (got[off:off + n_pos] == _bits(_written_out(call, k))).all(), k
            if flag & rows.OVERFLOW:
                assert (got[off:off + n_pos] == _bits(call["f"])).all() and call["counts"][k] > call["capacity"]
            seen.add((int(flag), int(call["counts"][k]) == call["capacity"], call["capacity"] == 0))
    # nothing flagged with a list that meets its capacity exactly; an overflow; a bad list; capacity 0 with and without hits
    assert {(0, True, False), (1, False, False), (2, False, False), (0, True, True), (1, False, True)} <= seen
    flags = cases.expected(cases.synthetic_calls()[1])[1]
    assert flags.tolist() == [0, 0, 1, 1, 2, 2, 2, 2, 0]


@pytest.mark.parametrize("method", METHODS)
def test_the_rule_on_the_cpu_equals_clamp_rows_host(check, tmp_path, method):
    rng = np.random.default_rng(11)
    row = (rng.random(5000, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    row[:6] = [-0.0, 0.0, np.nan, np.inf, -np.inf, 0.3]
    for clamp in (0.3, 0.0, -0.0, -0.4):
        f = axis.clamp_value(clamp, method)
        row[6] = f
        src, out = os.path.join(str(tmp_path), "in"), os.path.join(str(tmp_path), "out")
        row.tofile(src)
        subprocess.check_call([check, "clamp", method.split("_")[0], "%08x" % _b(f), src, out])
        assert (np.fromfile(out, np.uint32) == _bits(axis.clamp_rows_host(row, clamp, method))).all()


def test_rows_from_hits_host_refuses_bad_arguments():
    call = cases.synthetic_calls()[2]
    out = np.zeros(call["n_out"], np.float32)
    rows.rows_from_hits_host(call["hits"], call["counts"], call["table"], call["f"], out)
    with pytest.raises(SushiError):
        rows.rows_from_hits_host(call["hits"], call["counts"], call["table"], call["f"], out[:100])         # a row leaves the output
    with pytest.raises(SushiError):
        rows.rows_from_hits_host(call["hits"], call["counts"][:2], call["table"], call["f"], out)
    with pytest.raises(SushiError):
        rows.rows_from_hits_host(call["hits"], call["counts"], call["table"], np.float32(np.nan), out)
    with pytest.raises(SushiError):
        rows.rows_from_hits_host(call["hits"], call["counts"], call["table"], call["f"], out.astype(np.float64))


# ---------------------------------------------------------------------------------------------- the entry points, no GPU
def test_entry_points_refuse_bad_arguments_on_the_host():
    L = _native.lib()
    assert {"sushi_hip_rows_tile", "sushi_hip_rows_bytes", "sushi_hip_rows_from_hits", "sushi_hip_rows_clamp"} <= set(_native.declared_symbols())
    assert L.sushi_hip_rows_tile() == rows.TILE == 4096
    assert L.sushi_hip_rows_bytes(1) == 256 and L.sushi_hip_rows_bytes(9) == 512 and L.sushi_hip_rows_bytes(0) == 0 and \
        L.sushi_hip_rows_bytes(-3) == 0
    table = rows.rows_table([1, 7, 5001], [5, 4096, 12293], in_off=[1, 7, 5001])
    P = ctypes.c_void_p(1 << 20)                       # aligned, never dereferenced: every call below is refused first
    Q = ctypes.c_void_p(1 << 24)
    EINVAL, EALIGN = -1, -2

    def form(hits=P, counts=P, n=3, capacity=8, table=table, f=0.5, out=P, n_out=20000, flags=P, mem=P, mem_bytes=1 << 16):
        return L.sushi_hip_rows_from_hits(hits, counts, n, capacity, None if table is None else table.ctypes.data, f, out, n_out, flags,
                                          mem, mem_bytes, None)

    for name in ("hits", "counts", "table", "out", "flags", "mem"):
        assert form(**{name: None}) == EINVAL, name
    assert form(n=0) == EINVAL and form(n=-1) == EINVAL and form(capacity=-1) == EINVAL and form(n_out=0) == EINVAL
    assert form(f=float("nan")) == EINVAL and form(f=float("inf")) == EINVAL
    assert form(n_out=17293) == EINVAL and form(n_out=17294, mem_bytes=0) == _native.ENOSPACE
    for field, at, value in (("n_pos", 0, 0), ("n_pos", 1, -1), ("out_off", 0, -1), ("out_off", 2, 7708), ("out_off", 2, 2 ** 63 - 1)):
        bad = table.copy()
        bad[field][at] = value
        assert form(table=bad) == EINVAL, (field, at, value)
    assert form(mem=ctypes.c_void_p((1 << 20) + 128)) == EALIGN and form(counts=ctypes.c_void_p((1 << 20) + 4)) == EALIGN
    for name in ("hits", "out", "flags"):
        assert form(**{name: ctypes.c_void_p((1 << 20) + 2)}) == EALIGN, name
    assert form(mem_bytes=255) == _native.ENOSPACE

    def clamp(src=P, n_in=20000, out=Q, n_out=20000, table=table, n=3, method=0, f=0.5, mem=P, mem_bytes=1 << 16):
        return L.sushi_hip_rows_clamp(src, n_in, out, n_out, None if table is None else table.ctypes.data, n, method, f, mem, mem_bytes, None)

    for name in ("src", "out", "table", "mem"):
        assert clamp(**{name: None}) == EINVAL, name
    assert clamp(method=2) == EINVAL and clamp(method=-1) == EINVAL and clamp(n=0) == EINVAL and clamp(f=float("-inf")) == EINVAL
    assert clamp(n_in=0) == EINVAL and clamp(n_out=0) == EINVAL and clamp(n_in=17293) == EINVAL and clamp(n_out=17293) == EINVAL
    moved = table.copy()
    moved["in_off"][1] = 8
    assert clamp(out=P, mem_bytes=0) == _native.ENOSPACE            # in place is taken: the workspace is what fails
    assert clamp(out=P, table=moved) == EINVAL                      # the same buffer with a row moved
    assert clamp(out=ctypes.c_void_p((1 << 20) + 4)) == EINVAL      # buffers one float apart
    assert clamp(table=moved, mem_bytes=0) == _native.ENOSPACE      # apart: any offsets
    assert clamp(src=ctypes.c_void_p((1 << 20) + 2)) == EALIGN and clamp(mem=ctypes.c_void_p((1 << 20) + 64)) == EALIGN
    assert clamp(mem_bytes=255) == _native.ENOSPACE


# ---------------------------------------------------------------------------------------------- clamp= / capacity= of the searches
def _searches():
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    pcm = synth.make_dst_pcm(2, 12000, seed=1)
    dst = WavStream.from_samples(pcm, 12000, sample_type="uint8")
    pats, centres = [dst.get_substream(0.5, 0.7), dst.get_substream(1.0, 1.2)], [0.5, 1.0]
    return dst, [
        ("find_joint", lambda **kw: dst.find_joint(pats, centres, 0.1, **kw)),
        ("find_joint_many", lambda **kw: dst.find_joint_many([(pats, centres)], [0.1], **kw)),
        ("find_segments", lambda **kw: dst.find_segments(pats, centres, 0.1, 0.5, **kw)),
        ("find_drift", lambda **kw: dst.find_drift(pats, centres, 0.1, 1e-3, **kw)),
        ("find_track", lambda **kw: dst.find_track(pats, centres, 0.1, 0.5, reach=2, **kw))]


def test_the_searches_check_clamp_and_capacity_before_anything_else_runs():
    """No GPU here: with clamp=None the searches fail as they always did (a SushiError that names the missing GPU, or the error of the
    library that is not there); with clamp= the arguments are checked first -- before this feature the call itself was a TypeError."""
    import torch
    dst, searches = _searches()
    for name, call in searches:
        for bad in (dict(clamp=float("nan")), dict(clamp=float("inf")), dict(clamp="high"), dict(clamp=0.5, capacity=-1),
                    dict(clamp=0.5, capacity=2.5), dict(clamp=0.5, capacity=True), dict(capacity=100)):
            with pytest.raises(SushiError) as e:
                call(**bad)
            assert "clamp" in str(e.value) or "capacity" in str(e.value), (name, bad)
        if not torch.cuda.is_available():
            for kw in (dict(), dict(clamp=None), dict(clamp=0.5), dict(clamp=0.5, capacity=0)):
                with pytest.raises(SushiError) as e:
                    call(**kw)
                assert "clamp" not in str(e.value) and "capacity" not in str(e.value), (name, kw)


def test_default_capacity_is_bounded():
    assert axis.default_capacity(64, 2880001) == 2880001 // 16
    assert axis.default_capacity(7, 12001) == 1024 and axis.default_capacity(7, 500) == 500 and axis.default_capacity(1, 1) == 1
    assert axis.default_capacity(3000, 2880001) == axis.HIT_BYTES // (8 * 3000) and 8 * 3000 * axis.default_capacity(3000, 2880001) <= 256 << 20
    assert axis.checked_clamp(None, None, "sqdiff_normed") == (None, None)
    f, cap = axis.checked_clamp(0.7, 12, "ccoeff_normed")
    assert _bits(f) == _bits(np.float32(0.7)) and cap == 12


# ---------------------------------------------------------------------------------------------- the stream scenario on the oracle
@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_the_scenario_has_sparse_dense_and_empty_rows(oracle, sample_type):
    """What the GPU test of event_rows needs so that it cannot pass vacuously, shown on the CPU oracle's rows: at the chosen clamp
    at least two events whose hits fit the explicit capacity, the twice-planted event's do not, and the absent event has none."""
    import segment_cases
    dst, src = cases.streams(sample_type)
    patterns, centres = cases.scenario(dst, src)
    bases = [dst._get_sample_for_time(c) for c in centres]
    assert axis.joint_window(bases, [p.shape[1] for p in patterns], dst.data.shape[1], int(cases.RATE * cases.WINDOW)) == \
        (cases.K_LO, cases.N_SHIFT)
    for method in METHODS:
        found = segment_cases.oracle_rows(oracle, dst, patterns, bases, cases.K_LO, cases.N_SHIFT, method=method)
        f = axis.clamp_value(cases.CLAMPS[method], method)
        counts = [int(((r >= f) if method == "ccoeff_normed" else (r <= f)).sum()) for r in found]
        cap = cases.CAPACITY[method]
        assert counts[cases.TWICE] > cap and counts[cases.ABSENT] == 0
        assert sum(0 < c <= cap for c in counts) >= 2 and all(c <= cap for i, c in enumerate(counts) if i != cases.TWICE)
        if sample_type == "uint8":                      # (exact integer sums: the same counts everywhere)
            assert counts == cases.HITS[method]
        clamped = axis.clamp_rows_host(np.stack(found), cases.CLAMPS[method], method)
        assert [int((row != f).sum()) for row in clamped] == [c - int((r == f).sum()) for c, r in zip(counts, found)]
        keep = [axis.first_extremum(row, method) for row in clamped]
        assert keep[cases.ABSENT] == 0 and clamped[cases.ABSENT, 0] == f        # nothing passed: f at index 0
        assert keep[0] + cases.K_LO == cases.OFFSET
