"""Every occurrence of a pattern: the positions whose match score passes a threshold (``np.where(result >= t)`` on
``cv2.matchTemplate``'s row), without forming the row.

``find_occurrences`` runs a threshold run of an FFT-path batch (``SearchBatch.occurrences``, ``sushi_hip_batch_run_threshold``):
block pairs that no exact score can make pass are excluded by the pair bound, every position of the others is evaluated exactly
(DESIGN.md §3.10).  ``peaks`` thins the hits of one request to one per occurrence, on the host.

``find_best`` answers the question without a threshold: the K best distinct matches of every request, best first, from a best-K run
(``SearchBatch.best``, ``sushi_hip_batch_run_best``).  ``best_peaks`` is its reference on the host, over a curve.
"""
import numpy as np

from .axis import method_code
from .common import SushiError
from .device import SearchBatch, _checked_requests


def _fft_batch(dst, src, tmpl_off, tmpl_len, win_start, n_pos, method, threshold):
    """The argument checks find_occurrences and find_best share, and the FFT-path batch of their requests."""
    method_code(method)
    if dst.device != src.device:
        raise SushiError("dst and src streams live on different devices")
    if dst.dtype != src.dtype:
        raise SushiError("pattern and stream sample types differ (cv2.matchTemplate asserts equal types)")
    if threshold is not None and not np.isfinite(float(threshold)):
        raise SushiError("threshold must be finite")
    req = _checked_requests(dst, src, tmpl_off, tmpl_len, win_start, n_pos)
    return SearchBatch(dst, src, req["tmpl_off"], req["tmpl_len"], req["win_start"], req["n_pos"], path="fft", method=method)


def find_occurrences(dst, src, tmpl_off, tmpl_len, win_start, n_pos, threshold, method="ccoeff_normed", capacity=None):
    """Hits of a batch of requests (the arrays of ``SearchBatch``) on the DeviceStreams ``dst`` / ``src``: a list of
    ``(index int64 ndarray, score float32 ndarray)`` per request, in ascending index order.  method 'ccoeff_normed' (default):
    score >= threshold, the TM_CCOEFF_NORMED value itself; 'sqdiff_normed': score <= threshold.  Every score is bit-identical to
    ``match_curves`` at that index.  capacity: hits kept per request in a first pass (SearchBatch.occurrences)."""
    threshold = float(threshold)
    return _fft_batch(dst, src, tmpl_off, tmpl_len, win_start, n_pos, method, threshold).occurrences(threshold, capacity)


def peaks(index, score, min_separation, method="ccoeff_normed"):
    """Greedy suppression of the hits of one request: the best score first (the highest for 'ccoeff_normed', the lowest for
    'sqdiff_normed'; ties by the lower index), and a hit is kept only if no kept hit lies within ``min_separation`` positions
    (|i - j| < min_separation: a hit exactly min_separation away is kept).  Returns (index int64, score float32) of the kept hits
    in ascending index order.  Deterministic; NumPy on the host."""
    method_code(method)
    index = np.asarray(index, np.int64).reshape(-1)
    score = np.asarray(score, np.float32).reshape(-1)
    if index.shape != score.shape:
        raise SushiError("index and score must have the same length")
    sep = int(min_separation)
    if sep < 0:
        raise SushiError("min_separation must be >= 0")
    key = -score.astype(np.float64) if method == "ccoeff_normed" else score.astype(np.float64)
    order = np.lexsort((index, key))             # best score first, then the lower index
    kept = []
    kept_sorted = []                             # kept indices, ascending (binary search for the nearest)
    for j in order:
        i = int(index[j])
        pos = int(np.searchsorted(kept_sorted, i))
        if pos > 0 and i - kept_sorted[pos - 1] < sep:
            continue
        if pos < len(kept_sorted) and kept_sorted[pos] - i < sep:
            continue
        kept_sorted.insert(pos, i)
        kept.append(j)
    kept = np.asarray(sorted(kept, key=lambda j: int(index[j])), np.int64)
    return index[kept].astype(np.int64), score[kept].astype(np.float32)


def find_best(dst, src, tmpl_off, tmpl_len, win_start, n_pos, k, min_separation=None, threshold=None, method="ccoeff_normed"):
    """The k best distinct matches of every request (the arrays of ``SearchBatch``) on the DeviceStreams ``dst`` / ``src``: a list
    of ``(index int64 ndarray, score float32 ndarray)`` per request, best first -- ``best_peaks`` of the request's curve, without
    forming it.  min_separation: positions between two picks (None: the request's tmpl_len); threshold: only positions that pass
    it (score >= threshold for 'ccoeff_normed', <= for 'sqdiff_normed').  Every score is bit-identical to ``match_curves`` at
    that index.  A k beyond the number of real occurrences costs an exact evaluation of most of the window unless a threshold
    keeps chance-level scores out (SearchBatch.run_best)."""
    return _fft_batch(dst, src, tmpl_off, tmpl_len, win_start, n_pos, method, threshold).best(k, min_separation, threshold)


def best_peaks(curve, k, min_separation, method="ccoeff_normed", threshold=None):
    """The first k picks of greedy suppression over one score row: k masked arg-extrema.  Pick after pick, the best float32 score
    (the highest for 'ccoeff_normed', the lowest for 'sqdiff_normed'; ties by the lower index) among the positions that pass
    ``threshold`` (if given: score >= threshold / score <= threshold) and lie at least ``min_separation`` away from every earlier
    pick.  Returns (index int64, score float32) in pick order, best first; fewer than k where nothing is left.  This is ``peaks``
    over all eligible positions, sorted best first and cut at k.  NumPy on the host; needs no GPU."""
    method_code(method)
    c = np.asarray(curve, np.float32).reshape(-1)
    k = int(k)
    sep = int(min_separation)
    if k < 1:
        raise SushiError("k must be >= 1")
    if sep < 1:
        raise SushiError("min_separation must be >= 1")
    cc = method == "ccoeff_normed"
    free = np.ones(c.shape, bool)
    if threshold is not None:
        free &= (c.astype(np.float64) >= float(threshold)) if cc else (c.astype(np.float64) <= float(threshold))
    worst = np.float32(-np.inf) if cc else np.float32(np.inf)
    idx = []
    for _ in range(k):
        if not free.any():
            break
        masked = np.where(free, c, worst)
        g = int(np.argmax(masked)) if cc else int(np.argmin(masked))     # (the first of equal values: the lower index)
        if not free[g]:                                                   # (only scores as bad as the mask's are left: ties, the first of them)
            g = int(np.flatnonzero(free)[0])
        idx.append(g)
        free[max(0, g - sep + 1):g + sep] = False
    idx = np.asarray(idx, np.int64)
    return idx, c[idx].astype(np.float32)
