"""Whole match-score curves: the row ``cv2.matchTemplate`` returns (wav.py:185 ``result``), for any batch of searches.

``match_curves`` is the stateless counterpart of ``SearchBatch``: no batch handle, no spectra (the streams need not be
searchable), one call of ``sushi_hip_match_curves`` (include/sushi_hip.h).  Every value is bit-identical to what the exact
stages of a search produce at that position.
"""
import numpy as np
import torch

from . import _native
from .common import SushiError
from .device import _buffer, _checked_requests, _raw_stream


def match_curves(dst, src, tmpl_off, tmpl_len, win_start, n_pos, method="sqdiff_normed", out=None, hip_stream=None):
    """Curves of a batch of requests (the arrays of ``SearchBatch``) on the DeviceStreams ``dst`` / ``src``.

    Returns ``(curves, offsets)``: ``curves`` a flat float32 CUDA tensor on dst's device, request k's curve being
    ``curves[offsets[k]:offsets[k + 1]]``; ``offsets`` an int64 ndarray of n + 1 entries.  method: 'sqdiff_normed' (the
    TM_SQDIFF_NORMED value) or 'ccoeff_normed' (the TM_CCOEFF_NORMED value itself, not 1 - value).  ``out``: a contiguous
    float32 CUDA tensor of at least offsets[-1] elements to write into.  Asynchronous on ``hip_stream`` (default: the
    current torch stream of dst's device)."""
    if method not in _native.METHODS:
        raise SushiError("method must be one of %s" % sorted(_native.METHODS))
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
    with torch.cuda.device(dst.device):
        if out is None:
            out = torch.empty(total, dtype=torch.float32, device=dst.device)
        elif out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous() or out.numel() < total or \
                out.device != dst.device:
            raise SushiError("out: a contiguous float32 CUDA tensor of >= %d elements on %s" % (total, dst.device))
        mem = _buffer(max(256, L.sushi_hip_curve_bytes(req.ctypes.data, n)), dst.device)
        st = _raw_stream(dst.device) if hip_stream is None else hip_stream
        rc = L.sushi_hip_match_curves(dst.handle, src.handle, req.ctypes.data, n, _native.METHODS[method], mem.data_ptr(),
                                      mem.numel(), out.data_ptr(), st)
        _native.check(rc, "sushi_hip_match_curves")
        if hip_stream is not None:
            # (the workspace is the current stream's block: another stream's call returns it to the allocator only once passed)
            mem.record_stream(torch.cuda.ExternalStream(hip_stream, device=dst.device))
    return out, offsets
