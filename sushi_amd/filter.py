"""Filtering a stream before matching: mains hum, DC wander and rumble, or a dub's own speech, correlate with
themselves and hide what two streams share; a FIR filter applied to source and destination alike takes the band out and leaves
the shifts where they were.

* ``filter_host`` / ``filter_device`` -- a row through T float64 taps in the arithmetic of ``sushi_hip_filter``
  (include/sushi_hip.h): NumPy on the host, one kernel launch on the GPU, bit for bit the same.  ``WavStream.filtered`` makes a
  live stream of it.
* ``band_taps`` / ``preemphasis_taps`` -- the taps: Blackman-windowed sinc low-pass, high-pass, band-pass and band-stop; the
  pre-emphasis ``[-mu, 1, 0]``.  Host only.
"""
import numpy as np

from . import _native
from .common import SushiError
from .rowcheck import device_out, device_row, host_row, row_span

MAX_TAPS = 2047                                      # T: odd, 1 .. 2047 (sushi_hip_filter)

_HOST_OUTPUTS = 1 << 18      # outputs formed per NumPy pass of filter_host (bounds its temporaries)


def _check(n_in, in_start, n_taps, out_len):
    """The checks of sushi_hip_filter on Python integers; returns in_start and out_len as ints."""
    in_start, out_len = int(in_start), int(out_len)
    if not 1 <= n_taps <= MAX_TAPS or not n_taps & 1:
        raise SushiError("filter: an odd number of taps in 1..2047")
    row_span("filter", n_in, in_start, out_len)
    return in_start, out_len


def _host_taps(taps):
    """taps as a contiguous 1-D float64 array, finite (SushiError otherwise)."""
    h = np.ascontiguousarray(np.asarray(taps, dtype=np.float64))
    if h.ndim != 1 or not np.isfinite(h).all():
        raise SushiError("filter: taps must be a 1-D sequence of finite numbers")
    return h


def filter_host(samples, in_start, taps, out_len):
    """sushi_hip_filter in NumPy (include/sushi_hip.h states the arithmetic), and the CPU path.  With T taps h, a = (T - 1) // 2
    and c the sample type's centre (128 / 0.5): d(g) = float64(x[clip(g, 0, n - 1)]) - c; output i is the float64 running sum from
    0.0 over k = 0 .. T - 1, in that order, of h[k] * d(in_start + i + k - a), the product and the sum rounding separately.
    float32: float32(acc + 0.5); uint8: floor(acc + 128.5) held to 0 .. 255 (a NaN gives 0).  samples: a 1-D uint8 / float32
    array.  Returns out_len samples of its dtype."""
    x = host_row("filter", samples)
    h = _host_taps(taps)
    n, n_taps = x.shape[0], h.shape[0]
    in_start, out_len = _check(n, in_start, n_taps, out_len)
    a = (n_taps - 1) // 2
    u8 = x.dtype == np.uint8
    out = np.empty(out_len, x.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for i0 in range(0, out_len, _HOST_OUTPUTS):
            n_out = min(_HOST_OUTPUTS, out_len - i0)
            idx = np.clip(np.arange(in_start + i0 - a, in_start + i0 - a + n_out + n_taps - 1, dtype=np.int64), 0, n - 1)
            d = x[idx].astype(np.float64) - (128.0 if u8 else 0.5)
            acc = np.zeros(n_out, np.float64)
            for k in range(n_taps):                           # sequential in k: the kernel's order
                acc = acc + h[k] * d[k:k + n_out]
            if u8:
                v = np.floor(acc + 128.5)
                out[i0:i0 + n_out] = np.where(v >= 255.0, 255.0, np.where(v >= 0.0, v, 0.0)).astype(np.uint8)
            else:
                out[i0:i0 + n_out] = (acc + 0.5).astype(np.float32)
    return out


def filter_device(tensor, in_start, taps, out_len, out=None, hip_stream=None):
    """One call of sushi_hip_filter on a contiguous 1-D uint8 / float32 CUDA tensor.  taps: a sequence or NumPy array (checked for
    being finite and uploaded here) or a contiguous 1-D float64 CUDA tensor on the tensor's device (checked here too: one
    reduction and a wait for it).  out: a contiguous 1-D CUDA tensor (or view) of the same dtype and device with out_len samples
    to write into; None: a new one.  Asynchronous on hip_stream (default: the current torch stream of the tensor's device)."""
    import torch
    from .device import _launch
    code = device_row("filter", tensor)
    dev = tensor.device
    if isinstance(taps, torch.Tensor):
        if taps.dim() != 1 or taps.dtype != torch.float64 or taps.device != dev or not taps.is_contiguous():
            raise SushiError("filter: taps on the device must be a contiguous 1-D float64 tensor on the input's device")
        if taps.shape[0] and not bool(torch.isfinite(taps).all()):
            raise SushiError("filter: taps must be a 1-D sequence of finite numbers")
        h = taps
    else:
        h = torch.from_numpy(_host_taps(taps)).to(dev)       # (a blocking copy: done before a call on any stream)
    n, n_taps = int(tensor.shape[0]), int(h.shape[0])
    in_start, out_len = _check(n, in_start, n_taps, out_len)
    L = _native.lib()
    if out is None:
        out = torch.empty(out_len, dtype=tensor.dtype, device=dev)
    else:
        device_out("filter", tensor, out, out_len)
    _launch("sushi_hip_filter", dev, None,
            lambda mem, mem_bytes, st: L.sushi_hip_filter(tensor.data_ptr(), code, n, in_start, h.data_ptr(), n_taps,
                                                          out.data_ptr(), out_len, st),
            (tensor, h, out), hip_stream)
    return out


# ---------------------------------------------------------------------------------------------- the taps
def band_taps(rate, low=None, high=None, n_taps=255, stop=False):
    """n_taps float64 Blackman-windowed sinc taps at sample rate `rate` (Hz).  With a = (n_taps - 1) // 2, k = arange(n_taps) - a
    and w the Blackman window, lp(f) = 2 (f / rate) sinc(2 (f / rate) k) w divided by its own sum (gain 1 at DC).  Only high:
    the low-pass lp(high).  Only low: the high-pass delta - lp(low).  Both: the band-pass lp(high) - lp(low).  stop=True: delta
    minus that (only high: a high-pass; only low: a low-pass; both: a band-stop).  Symmetric, so linear in phase and without a
    shift of its own.  SushiError: n_taps even or outside 3 .. 2047, neither edge given, edges outside 0 < low < high < rate / 2."""
    n_taps = int(n_taps)
    if not 3 <= n_taps <= MAX_TAPS or not n_taps & 1:
        raise SushiError("band_taps: an odd number of taps in 3..2047")
    if low is None and high is None:
        raise SushiError("band_taps: give low, high or both")
    rate = float(rate)
    edges = [float(f) for f in (low, high) if f is not None]
    if not rate > 0 or any(not 0.0 < f < rate / 2.0 for f in edges) or (len(edges) == 2 and not edges[0] < edges[1]):
        raise SushiError("band_taps: edges must satisfy 0 < low < high < rate / 2")
    a = (n_taps - 1) // 2
    k = np.arange(n_taps, dtype=np.float64) - a
    w = np.blackman(n_taps)
    delta = np.zeros(n_taps, np.float64)
    delta[a] = 1.0

    def lp(f):
        h = 2.0 * (f / rate) * np.sinc(2.0 * (f / rate) * k) * w
        return h / h.sum()

    if low is None:
        h = lp(float(high))
    elif high is None:
        h = delta - lp(float(low))
    else:
        h = lp(float(high)) - lp(float(low))
    return delta - h if stop else h


def preemphasis_taps(mu=0.97):
    """[-mu, 1.0, 0.0]: output i is x[i] - mu * x[i - 1] about the centre -- programme material whose energy lies at the bottom
    of the band gets sharper score minima."""
    mu = float(mu)
    if not np.isfinite(mu):
        raise SushiError("preemphasis_taps: mu must be finite")
    return np.array([-mu, 1.0, 0.0], np.float64)
