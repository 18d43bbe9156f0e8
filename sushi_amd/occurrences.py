"""Every occurrence of a pattern: the positions whose match score passes a threshold (``np.where(result >= t)`` on
``cv2.matchTemplate``'s row), without forming the row.

``find_occurrences`` runs a threshold run of an FFT-path batch (``SearchBatch.occurrences``, ``sushi_hip_batch_run_threshold``):
block pairs that no exact score can make pass are excluded by the pair bound, every position of the others is evaluated exactly
(DESIGN.md §3.10).  ``peaks`` thins the hits of one request to one per occurrence, on the host.
"""
import numpy as np

from . import _native
from .common import SushiError
from .device import SearchBatch, _checked_requests


def find_occurrences(dst, src, tmpl_off, tmpl_len, win_start, n_pos, threshold, method="ccoeff_normed", capacity=None):
    """Hits of a batch of requests (the arrays of ``SearchBatch``) on the DeviceStreams ``dst`` / ``src``: a list of
    ``(index int64 ndarray, score float32 ndarray)`` per request, in ascending index order.  method 'ccoeff_normed' (default):
    score >= threshold, the TM_CCOEFF_NORMED value itself; 'sqdiff_normed': score <= threshold.  Every score is bit-identical to
    ``match_curves`` at that index.  capacity: hits kept per request in a first pass (SearchBatch.occurrences)."""
    if method not in _native.METHODS:
        raise SushiError("method must be one of %s" % sorted(_native.METHODS))
    if dst.device != src.device:
        raise SushiError("dst and src streams live on different devices")
    if dst.dtype != src.dtype:
        raise SushiError("pattern and stream sample types differ (cv2.matchTemplate asserts equal types)")
    threshold = float(threshold)
    if not np.isfinite(threshold):
        raise SushiError("threshold must be finite")
    req = _checked_requests(dst, src, tmpl_off, tmpl_len, win_start, n_pos)
    batch = SearchBatch(dst, src, req["tmpl_off"], req["tmpl_len"], req["win_start"], req["n_pos"], path="fft", method=method)
    return batch.occurrences(threshold, capacity)


def peaks(index, score, min_separation, method="ccoeff_normed"):
    """Greedy suppression of the hits of one request: the best score first (the highest for 'ccoeff_normed', the lowest for
    'sqdiff_normed'; ties by the lower index), and a hit is kept only if no kept hit lies within ``min_separation`` positions
    (|i - j| < min_separation: a hit exactly min_separation away is kept).  Returns (index int64, score float32) of the kept hits
    in ascending index order.  Deterministic; NumPy on the host."""
    if method not in _native.METHODS:
        raise SushiError("method must be one of %s" % sorted(_native.METHODS))
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
