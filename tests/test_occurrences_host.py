"""Threshold runs (sushi_hip_batch_run_threshold, sushi_amd.occurrences, WavStream.find_occurrences): the host side -- the C ABI's
symbol, record type and argument checks before any HIP call, peak picking, the widest window.  No GPU needed."""
import ctypes

import numpy as np
import pytest

from sushi_amd import _native
from sushi_amd.common import SushiError
from sushi_amd.occurrences import peaks

C = ctypes


def test_threshold_symbol_is_declared_exported_and_typed():
    assert "sushi_hip_batch_run_threshold" in _native.declared_symbols()
    L = _native.lib()
    f = L.sushi_hip_batch_run_threshold
    assert f.restype is C.c_int and len(f.argtypes) == 6
    assert f.argtypes[1] is C.c_double and f.argtypes[2] is C.c_int32
    assert L.sushi_hip_abi_version() == 13


def test_hit_dtype_is_the_c_struct():
    class Hit(C.Structure):
        _fields_ = [("index", C.c_int32), ("score", C.c_float)]
    assert _native.HIT_DTYPE.itemsize == C.sizeof(Hit) == 8
    assert _native.HIT_DTYPE.names == ("index", "score")
    assert _native.HIT_DTYPE.fields["index"][1] == Hit.index.offset == 0
    assert _native.HIT_DTYPE.fields["score"][1] == Hit.score.offset == 4
    rec = np.zeros(2, _native.HIT_DTYPE)
    rec["index"], rec["score"] = [3, 7], [0.5, -0.25]
    raw = rec.view(np.int32).reshape(2, 2)           # the (index, score bits) int32 pairs SearchBatch.run_threshold returns
    assert raw[1, 0] == 7 and raw[1, 1].view(np.float32) == np.float32(-0.25)
    with open(_native.HEADER_PATH) as f:
        text = f.read()
    assert "typedef struct SushiHipHit" in text and "int32_t index;" in text and "float score;" in text


def test_threshold_arguments_rejected_before_any_hip_call():
    L = _native.lib()
    fake = C.c_void_p(4096)                 # never dereferenced: every check below fails before the batch is read
    hits, counts = C.c_void_p(8192), C.c_void_p(16384)
    f = L.sushi_hip_batch_run_threshold
    assert f(None, 0.5, 16, hits, counts, None) == -1
    assert f(fake, 0.5, 16, None, counts, None) == -1
    assert f(fake, 0.5, 16, hits, None, None) == -1
    assert f(fake, 0.5, -1, hits, counts, None) == -1
    for t in (float("nan"), float("inf"), float("-inf")):
        assert f(fake, t, 16, hits, counts, None) == -1
    assert f(None, float("nan"), -5, None, None, None) == -1


def test_peaks_best_first_ties_by_lower_index():
    idx = np.array([10, 11, 12, 13, 40, 41, 100], np.int64)
    sc = np.array([0.5, 0.9, 0.9, 0.7, 0.8, 0.8, 0.6], np.float32)
    i, s = peaks(idx, sc, 5, "ccoeff_normed")
    # 11 and 12 tie: 11 (lower index) is kept and 12 goes; 40 / 41 tie: 40 kept; 100 alone
    assert i.tolist() == [11, 40, 100] and s.dtype == np.float32 and s.tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.6)]
    # sqdiff: the LOWEST score first (10, then 100; 13 lies within 5 of 10; 40 / 41 tie: 40)
    i, s = peaks(idx, sc, 5, "sqdiff_normed")
    assert i.tolist() == [10, 40, 100]
    assert peaks(idx, sc, 5, "sqdiff_normed")[1].tolist() == [np.float32(0.5), np.float32(0.8), np.float32(0.6)]


def test_peaks_at_exactly_min_separation_are_both_kept():
    idx = np.array([0, 5, 10, 14], np.int64)
    sc = np.array([0.9, 0.9, 0.9, 0.95], np.float32)
    # 14 first; 10 is 4 away (< 5): dropped; 0 next (ties by index), 5 exactly 5 from 0 and 9 from 14: kept
    assert peaks(idx, sc, 5, "ccoeff_normed")[0].tolist() == [0, 5, 14]
    assert peaks(idx, sc, 6, "ccoeff_normed")[0].tolist() == [0, 14]
    # 0 keeps everything, equal scores everywhere: order by index
    assert peaks(idx, np.full(4, 0.3, np.float32), 0, "sqdiff_normed")[0].tolist() == [0, 5, 10, 14]
    assert peaks(idx, np.full(4, 0.3, np.float32), 1, "sqdiff_normed")[0].tolist() == [0, 5, 10, 14]


def test_peaks_is_deterministic_and_checks_its_arguments():
    rng = np.random.default_rng(0)
    idx = np.sort(rng.choice(10000, 500, replace=False)).astype(np.int64)
    sc = rng.random(500).astype(np.float32)
    a = peaks(idx, sc, 50, "ccoeff_normed")
    b = peaks(idx[::-1].copy(), sc[::-1].copy(), 50, "ccoeff_normed")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.all(np.diff(a[0]) >= 50)
    # every dropped hit lies within 50 of a kept hit that scores at least as well
    for i, s in zip(idx, sc):
        near = np.abs(a[0] - i) < 50
        assert near.any() and (a[1][near] >= s).any()
    assert peaks(np.zeros(0, np.int64), np.zeros(0, np.float32), 3)[0].size == 0
    with pytest.raises(SushiError):
        peaks(idx, sc[:3], 5)
    with pytest.raises(SushiError):
        peaks(idx, sc, -1)
    with pytest.raises(SushiError):
        peaks(idx, sc, 5, "sqdiff")


@pytest.mark.parametrize("sample_rate", [12000, 24000])
def test_the_widest_window_is_the_whole_stream(sample_rate):
    from sushi_amd.wav import WavStream
    seconds, pad = 7.25, WavStream.PADDING_SECONDS
    n = int(round((seconds + 2 * pad) * sample_rate))
    data = np.zeros((1, n), np.uint8)
    ws = WavStream.from_prepared(data, sample_rate, int(round(seconds * sample_rate)), pad * sample_rate)
    c, w = ws._widest(None, None)
    assert c == ws.duration_seconds / 2.0 and w == ws.duration_seconds / 2.0 + pad
    for m in (1, 100, 36000):
        start_time, lo, n_pos = ws._window(m, c, w)
        assert start_time == -pad and lo == 0 and n_pos == n - m + 1
    # a given centre or size is kept
    assert ws._widest(3.0, None) == (3.0, w) and ws._widest(None, 2.0) == (c, 2.0)


def test_occurrence_entry_points_exist():
    from sushi_amd import device, occurrences, wav
    assert callable(occurrences.find_occurrences) and callable(occurrences.peaks)
    assert callable(device.SearchBatch.run_threshold) and callable(device.SearchBatch.occurrences)
    assert callable(wav.WavStream.find_occurrences) and callable(wav.WavStream.find_occurrences_many)
