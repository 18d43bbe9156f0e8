"""Best-K runs (sushi_hip_batch_run_best, sushi_amd.occurrences.find_best / best_peaks, WavStream.find_best_matches): the host
side -- the C ABI's symbol and argument checks before any HIP call, the host reference of greedy suppression.  No GPU needed."""
import ctypes

import numpy as np
import pytest

from sushi_amd import _native
from sushi_amd.common import SushiError
from sushi_amd.occurrences import best_peaks, peaks

C = ctypes


def test_best_symbol_is_declared_exported_and_typed():
    assert "sushi_hip_batch_run_best" in _native.declared_symbols()
    L = _native.lib()
    f = L.sushi_hip_batch_run_best
    assert f.restype is C.c_int and len(f.argtypes) == 7
    assert f.argtypes[1] is C.c_int32 and f.argtypes[2] is C.c_int32 and f.argtypes[3] is C.POINTER(C.c_double)
    assert L.sushi_hip_abi_version() == 13
    with open(_native.HEADER_PATH) as fh:
        text = fh.read()
    assert "#define SUSHI_HIP_BEST_MAX_K 32" in text and "#define SUSHI_HIP_ABI_VERSION 13 " in text
    assert _native.BEST_MAX_K == 32


def test_best_arguments_rejected_before_any_hip_call():
    L = _native.lib()
    fake = C.c_void_p(4096)                 # never dereferenced: every check below fails before the batch is read
    hits, counts = C.c_void_p(8192), C.c_void_p(16384)
    f = L.sushi_hip_batch_run_best
    thr = C.byref(C.c_double(0.5))
    EINVAL, EALIGN = -1, -2
    assert f(None, 3, 0, None, hits, counts, None) == EINVAL
    assert f(fake, 3, 0, None, None, counts, None) == EINVAL
    assert f(fake, 3, 0, None, hits, None, None) == EINVAL
    for k in (0, -1, 33, 1 << 20):
        assert f(fake, k, 0, None, hits, counts, None) == EINVAL
        assert f(fake, k, 0, thr, hits, counts, None) == EINVAL
    assert f(fake, 3, -1, None, hits, counts, None) == EINVAL
    for t in (float("nan"), float("inf"), float("-inf")):
        assert f(fake, 3, 0, C.byref(C.c_double(t)), hits, counts, None) == EINVAL
        assert f(fake, 3, 100, C.byref(C.c_double(t)), hits, counts, None) == EINVAL
    assert f(None, 0, -5, C.byref(C.c_double(float("nan"))), None, None, None) == EINVAL


def test_best_peaks_pick_order_and_ties_by_lower_index():
    c = np.full(200, 0.1, np.float32)
    c[[11, 12]] = 0.9
    c[[40, 41]] = 0.8
    c[100] = 0.6
    c[13] = 0.7
    i, s = best_peaks(c, 3, 5, "ccoeff_normed")
    # 11 and 12 tie: 11; 13 lies within 5 of 11; 40 / 41 tie: 40; then 100
    assert i.dtype == np.int64 and s.dtype == np.float32
    assert i.tolist() == [11, 40, 100] and s.tolist() == [np.float32(0.9), np.float32(0.8), np.float32(0.6)]
    assert best_peaks(c, 1, 5, "ccoeff_normed")[0].tolist() == [11]
    # sqdiff: the LOWEST first
    d = (1.0 - c).astype(np.float32)
    assert best_peaks(d, 3, 5, "sqdiff_normed")[0].tolist() == [11, 40, 100]
    # the score itself orders the picks, not 1 - score: two coefficients that 1 - c merges in float32 stay apart
    e = np.zeros(50, np.float32)
    e[10], e[30] = np.float32(1e-9), np.float32(2e-9)
    assert np.float32(1) - e[10] == np.float32(1) - e[30]
    assert best_peaks(e, 2, 5, "ccoeff_normed")[0].tolist() == [30, 10]


def test_best_peaks_exactly_min_separation_away_is_kept():
    c = np.zeros(40, np.float32)
    c[[0, 5, 10]] = 0.9
    c[14] = 0.95
    # 14 first; 10 is 4 away (< 5): suppressed; 0 (ties by index), 5 exactly 5 from 0 and 9 from 14: kept
    assert best_peaks(c, 3, 5, "ccoeff_normed")[0].tolist() == [14, 0, 5]
    assert best_peaks(c, 3, 6, "ccoeff_normed")[0].tolist()[:2] == [14, 0]
    assert 5 not in best_peaks(c, 3, 6, "ccoeff_normed")[0].tolist()


def test_best_peaks_kth_score_is_not_monotone_in_the_positions_seen():
    # A 0.1 @10, B 0.2 @20, S = 8, K = 2 pick [10, 20]; C 0.05 @15 lies within S of both: the picks become C and the next best
    c = np.full(100, 1.0, np.float32)
    c[10], c[20], c[60] = 0.1, 0.2, 0.9
    assert best_peaks(c, 2, 8, "sqdiff_normed")[0].tolist() == [10, 20]
    c[15] = 0.05
    i, s = best_peaks(c, 2, 8, "sqdiff_normed")
    assert i.tolist() == [15, 60] and s.tolist() == [np.float32(0.05), np.float32(0.9)]


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
def test_best_peaks_constant_row_picks_every_sth_position(method):
    c = np.full(50, 0.25, np.float32)
    assert best_peaks(c, 4, 7, method)[0].tolist() == [0, 7, 14, 21]
    assert best_peaks(c, 32, 7, method)[0].tolist() == list(range(0, 50, 7))       # the row ends before k picks
    assert best_peaks(c[:1], 3, 7, method)[0].tolist() == [0]
    assert best_peaks(c, 3, 1, method)[0].tolist() == [0, 1, 2]


def test_best_peaks_threshold_cuts_the_list_short():
    c = np.zeros(300, np.float32)
    c[50], c[150], c[250] = 0.9, 0.7, 0.5
    assert best_peaks(c, 5, 10, "ccoeff_normed", threshold=0.6)[0].tolist() == [50, 150]
    assert best_peaks(c, 5, 10, "ccoeff_normed", threshold=float(np.float32(0.7)))[0].tolist() == [50, 150]    # equal passes
    assert best_peaks(c, 5, 10, "ccoeff_normed", threshold=0.95)[0].size == 0
    assert best_peaks(c, 1, 10, "ccoeff_normed", threshold=0.6)[0].tolist() == [50]
    d = (1.0 - c).astype(np.float32)
    assert best_peaks(d, 5, 10, "sqdiff_normed", threshold=0.4)[0].tolist() == [50, 150]
    assert best_peaks(d, 5, 10, "sqdiff_normed", threshold=0.05)[0].size == 0


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
def test_best_peaks_is_peaks_over_all_positions_best_first_cut_at_k(method):
    rng = np.random.default_rng(7)
    for trial in range(60):
        n = int(rng.integers(1, 400))
        levels = int(rng.integers(2, 12))                               # few distinct values: ties everywhere
        c = (rng.integers(0, levels, n) / np.float32(levels)).astype(np.float32)
        sep = int(rng.integers(1, 40))
        k = int(rng.integers(1, 33))
        thr = None if trial % 3 else float(c[int(rng.integers(0, n))])
        if thr is None:
            elig = np.arange(n, dtype=np.int64)
        else:
            elig = np.flatnonzero(c >= np.float32(thr) if method == "ccoeff_normed" else c <= np.float32(thr)).astype(np.int64)
        pi, ps = peaks(elig, c[elig], sep, method)
        key = -ps.astype(np.float64) if method == "ccoeff_normed" else ps.astype(np.float64)
        order = np.lexsort((pi, key))[:k]
        bi, bs = best_peaks(c, k, sep, method, threshold=thr)
        assert bi.tolist() == pi[order].tolist(), (trial, n, sep, k, thr)
        assert bs.view(np.uint32).tolist() == ps[order].view(np.uint32).tolist()


def test_best_peaks_checks_its_arguments():
    c = np.zeros(10, np.float32)
    with pytest.raises(SushiError):
        best_peaks(c, 0, 3)
    with pytest.raises(SushiError):
        best_peaks(c, 2, 0)
    with pytest.raises(SushiError):
        best_peaks(c, 2, 3, "sqdiff")
    assert best_peaks(np.zeros(0, np.float32), 2, 3)[0].size == 0


def test_best_entry_points_exist():
    from sushi_amd import device, occurrences, wav
    assert callable(occurrences.find_best) and callable(occurrences.best_peaks)
    assert callable(device.SearchBatch.run_best) and callable(device.SearchBatch.best)
    assert callable(wav.WavStream.find_best_matches) and callable(wav.WavStream.find_best_matches_many)
