"""Whole match-score curves: the row ``cv2.matchTemplate`` returns (wav.py:185 ``result``), for any batch of searches.

``match_curves`` is the stateless counterpart of ``SearchBatch``: no batch handle, no spectra (the streams need not be
searchable), one call of ``sushi_hip_match_curves`` (include/sushi_hip.h).  Every value is bit-identical to what the exact
stages of a search produce at that position.
"""
import numpy as np
import torch

from . import _native
from .axis import method_code
from .common import SushiError
from .device import _checked_requests, _launch


def match_curves(dst, src, tmpl_off, tmpl_len, win_start, n_pos, method="sqdiff_normed", out=None, hip_stream=None):
    """Curves of a batch of requests (the arrays of ``SearchBatch``) on the DeviceStreams ``dst`` / ``src``.

    Returns ``(curves, offsets)``: ``curves`` a flat float32 CUDA tensor on dst's device, request k's curve being
    ``curves[offsets[k]:offsets[k + 1]]``; ``offsets`` an int64 ndarray of n + 1 entries.  method: 'sqdiff_normed' (the
    TM_SQDIFF_NORMED value) or 'ccoeff_normed' (the TM_CCOEFF_NORMED value itself, not 1 - value).  ``out``: a contiguous
    float32 CUDA tensor of at least offsets[-1] elements to write into.  Asynchronous on ``hip_stream`` (default: the
    current torch stream of dst's device)."""
    code = method_code(method)
    if dst.device != src.device:
        raise SushiError("dst and src streams live on different devices")
    if dst.dtype != src.dtype:
        raise SushiError("pattern and stream sample types differ (cv2.matchTemplate asserts equal types)")
    req = _checked_requests(dst, src, tmpl_off, tmpl_len, win_start, n_pos)
    n = req.shape[0]
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(req["n_pos"].astype(np.int64), out=offsets[1:])
    total = int(offsets[-1])
    L = _native.lib()
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=dst.device)
    elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() < total or \
            out.device != dst.device:
        raise SushiError("out: a contiguous float32 CUDA tensor of >= %d elements on %s" % (total, dst.device))
    _launch("sushi_hip_match_curves", dst.device, L.sushi_hip_curve_bytes(req.ctypes.data, n),
            lambda mem, mem_bytes, st: L.sushi_hip_match_curves(dst.handle, src.handle, req.ctypes.data, n, code, mem, mem_bytes,
                                                                out.data_ptr(), st),
            (out, dst.raw, dst._mem, src.raw, src._mem), hip_stream)
    return out, offsets
