"""Levelling a stream before matching: a normalised score weights each instant by its energy, so where two
releases share a quiet bed under loud speech of their own -- two mono dubs -- the unrelated speech decides the score and the bed
in the pauses counts for nothing; a capture through an AGC or a broadcast compressor loses the same.  Every sample divided by the
local level, the mean absolute deviation over about 10 ms around it, lets the pauses count as much as the words.

* ``level_host`` / ``level_device`` -- a row levelled in the arithmetic of ``sushi_hip_level`` (include/sushi_hip.h): NumPy on
  the host, one kernel launch on the GPU, bit for bit the same.  ``WavStream.levelled`` makes a live stream of it.
"""
import math

import numpy as np

from . import _native
from .common import SushiError
from .rowcheck import device_out, device_row, host_row, row_span

MAX_WINDOW = 1023                                    # W: odd, 1 .. 1023 (sushi_hip_level)
WINDOW, FLOOR, PEAK = 129, 1.0 / 128, 8.0            # WavStream.levelled's defaults

_HOST_OUTPUTS = 1 << 18      # outputs formed per NumPy pass of level_host (bounds its temporaries)


def _check(n_in, in_start, window, floor, peak, out_len):
    """The checks of sushi_hip_level on Python numbers; returns them as ints and floats."""
    try:
        in_start, window, out_len, floor, peak = int(in_start), int(window), int(out_len), float(floor), float(peak)
    except (TypeError, ValueError):
        raise SushiError("level: window, floor and peak must be numbers")
    if not 1 <= window <= MAX_WINDOW or not window & 1:
        raise SushiError("level: an odd window in 1..1023")
    if not (math.isfinite(floor) and floor > 0.0 and math.isfinite(peak) and peak > 0.0):
        raise SushiError("level: floor and peak must be finite and > 0")
    row_span("level", n_in, in_start, out_len)
    return in_start, window, floor, peak, out_len


def level_host(samples, in_start, window, floor, peak, out_len):
    """sushi_hip_level in NumPy (include/sushi_hip.h states the arithmetic), and the CPU path.  With W = window, h = (W - 1) // 2,
    c and H the sample type's centre and half range (128, 128.0 / 0.5, 0.5) and d(j) = x[clip(j, 0, n - 1)] - c (uint8: an integer;
    float32: one float64 subtraction): for output i and g = in_start + i, E = the sum over t = 0 .. W - 1 of |d(g - h + t)| --
    uint8: exact; float32: a float64 running sum from 0.0 in that order; fw = (floor * H) * W; den = (E + fw) * peak;
    q = (d(g) * W) / den, a NaN made 0, then held to [-1, 1].  float32: float32(0.5 + 0.5 * q); uint8: min(255, floor(q * 128.0 +
    128.5)).  samples: a 1-D uint8 / float32 array.  Returns out_len samples of its dtype."""
    x = host_row("level", samples)
    n = x.shape[0]
    in_start, window, floor, peak, out_len = _check(n, in_start, window, floor, peak, out_len)
    h, w = (window - 1) // 2, float(window)
    u8 = x.dtype == np.uint8
    fw = (floor * (128.0 if u8 else 0.5)) * w
    out = np.empty(out_len, x.dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for i0 in range(0, out_len, _HOST_OUTPUTS):
            n_out = min(_HOST_OUTPUTS, out_len - i0)
            g0 = in_start + i0 - h
            idx = np.clip(np.arange(g0, g0 + n_out + window - 1, dtype=np.int64), 0, n - 1)
            if u8:
                d = x[idx].astype(np.int64) - 128
                p = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.abs(d))])
                e = (p[window:] - p[:n_out]).astype(np.float64)
            else:
                d = x[idx].astype(np.float64) - 0.5
                a = np.abs(d)
                e = np.zeros(n_out, np.float64)
                for t in range(window):                           # sequential in t: the kernel's order
                    e = e + a[t:t + n_out]
            den = (e + fw) * peak
            q = (d[h:h + n_out].astype(np.float64) * w) / den
            q = np.where(np.isnan(q), 0.0, q)
            q = np.where(q > 1.0, 1.0, np.where(q < -1.0, -1.0, q))
            if u8:
                out[i0:i0 + n_out] = np.minimum(np.floor(q * 128.0 + 128.5), 255.0).astype(np.uint8)
            else:
                out[i0:i0 + n_out] = (0.5 + 0.5 * q).astype(np.float32)
    return out


def level_device(tensor, in_start, window, floor, peak, out_len, out=None, hip_stream=None):
    """One call of sushi_hip_level on a contiguous 1-D uint8 / float32 CUDA tensor.  out: a contiguous 1-D CUDA tensor (or view)
    of the same dtype and device with out_len samples to write into; None: a new one.  Asynchronous on hip_stream (default: the
    current torch stream of the tensor's device)."""
    import torch
    from .device import _launch
    code = device_row("level", tensor)
    n = int(tensor.shape[0])
    in_start, window, floor, peak, out_len = _check(n, in_start, window, floor, peak, out_len)
    L = _native.lib()
    dev = tensor.device
    if out is None:
        out = torch.empty(out_len, dtype=tensor.dtype, device=dev)
    else:
        device_out("level", tensor, out, out_len)
    _launch("sushi_hip_level", dev, None,
            lambda mem, mem_bytes, st: L.sushi_hip_level(tensor.data_ptr(), code, n, in_start, window, floor, peak,
                                                         out.data_ptr(), out_len, st),
            (tensor, out), hip_stream)
    return out
