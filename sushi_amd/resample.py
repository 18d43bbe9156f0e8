"""A low-pass in front of the load pipeline's decimator (``WavStream(..., resample='fir')``).

The reference decimates by taking the nearest input frame (cv2.resize INTER_NEAREST, wav.py:125-137): whatever lies above half
the stream's sample rate folds into the stream at full level, and two files of one programme at different frame rates fold
differently.  ``'fir'`` puts a zero-phase windowed-sinc filter at the file's frame rate in front: body sample ``i`` is the
filter centred on input position ``i * num / den`` (``num / den`` = frame rate / sample rate in lowest terms), where the nearest
path reads the floor of that position, so the stream keeps its shape and its time axis.

* ``ratio`` / ``fir_table`` -- the step and the polyphase table (NumPy float64, built once per pair of rates on the host; the
  same table serves the CPU path and the kernel, so no libm difference can separate them);
* ``resample_host`` / ``resample_device`` -- the filter in the arithmetic of ``sushi_hip_load_resample_fir`` (include/sushi_hip.h):
  NumPy float64 on the host, one library call on the GPU, bit for bit the same.
"""
import functools
import math

import numpy as np

from . import _native
from .common import SushiError
from .row import fill_pads

ZEROS = 16                   # zero crossings of the sinc on each side of its centre
ROLLOFF = 0.9                # the cut-off as a fraction of the lower of the two Nyquist frequencies
MAX_TERM = 1 << 20           # num and den (sushi_hip_load_resample_fir)
MAX_TABLE = 65536            # den * 2W table entries
MAX_BODY = 1 << 40           # body samples
MODES = ('nearest', 'fir')


def check_mode(resample):
    if not isinstance(resample, str) or resample not in MODES:
        raise SushiError("resample must be 'nearest' or 'fir', not %r" % (resample,))
    return resample


def ratio(fr, sr):
    """(num, den): input frames per output sample, frame rate / sample rate in lowest terms."""
    fr, sr = int(fr), int(sr)
    if fr < 1 or sr < 1:
        raise SushiError('resample: rates must be positive integers')
    g = math.gcd(fr, sr)
    return fr // g, sr // g


@functools.lru_cache(maxsize=16)
def _table(num, den):
    fc = ROLLOFF * 0.5 * min(1.0, den / num)                 # cycles per input sample
    W = int(math.ceil(ZEROS / (2 * fc)))
    if not (1 <= num <= MAX_TERM and 1 <= den <= MAX_TERM) or den * 2 * W > MAX_TABLE:
        raise SushiError('resample: a step of %d / %d needs %d x %d table entries (at most %d, terms at most 2^20)'
                         % (num, den, den, 2 * W, MAX_TABLE))
    k = np.arange(-W + 1, W + 1, dtype=np.float64)           # column c is k = c - W + 1
    r = np.arange(den, dtype=np.float64)
    d = k[None, :] - r[:, None] / den
    h = np.sinc(2 * fc * d) * (0.5 + 0.5 * np.cos(np.pi * d / W))
    h = h / h.sum(axis=1, keepdims=True)
    h = np.ascontiguousarray(h, dtype=np.float64)
    h.setflags(write=False)
    return W, h


def fir_table(fr, sr):
    """(num, den, W, H): the step, the half width and the float64 table [den, 2W] of the filter that takes frame rate `fr` to
    sample rate `sr`.  Row r is the filter of an output that lies r / den behind an input frame: column c weighs the frame
    k = c - W + 1 frames from it, h = sinc(2 fc d) * (0.5 + 0.5 cos(pi d / W)) at d = k - r / den with
    fc = ROLLOFF * 0.5 * min(1, den / num) and W = ceil(ZEROS / (2 fc)); every row is divided by its own sum.  Read-only, cached.
    SushiError when the table would pass 65536 entries or a term 2^20."""
    num, den = ratio(fr, sr)
    W, h = _table(num, den)
    return num, den, W, h


_HOST_BLOCK = 1 << 18        # outputs per NumPy pass of resample_host (bounds its temporaries)


def _check_body(n_raw, num, den, n_body):
    if n_raw < 1 or n_body < 1 or n_body >= MAX_BODY:
        raise SushiError('resample: needs input frames and 1 .. 2^40 - 1 body samples')
    if (n_body - 1) * num // den > n_raw - 1:
        raise SushiError('resample: the last body sample lies behind the input')


def resample_host(samples, fr, sr, n_body, first=0, count=None, stride=1):
    """sushi_hip_load_resample_fir's body in NumPy (include/sushi_hip.h states the arithmetic), and the CPU path: for body sample i
    t = i * num (int64), j = t // den, r = t % den, acc = 0.0, then for c = 0 .. 2W - 1 in that order
    acc = acc + H[r][c] * float64(x[clip(j - W + 1 + c, 0, n - 1)]); the sample is float32(acc).
    samples: a 1-D float32 array of frames at rate `fr` (or an object with its ndim, dtype and shape that returns the float32
    frames at an int64 index array: an input too long to hold, computed from its index); n_body: the body's length (its last sample must not lie behind the
    input).  Returns body samples [first, first + count) as float32 (count=None: to the body's end; stride: every stride-th of them from
    `first` on, `count` in all).  fr == sr: a copy."""
    lazy = not isinstance(samples, np.ndarray) and all(hasattr(samples, a) for a in ('ndim', 'dtype', 'shape', '__getitem__'))
    x = samples if lazy else np.asarray(samples)
    if x.ndim != 1 or x.dtype != np.float32:
        raise SushiError('resample: a 1-D float32 array')
    n = x.shape[0]
    num, den = ratio(fr, sr)
    n_body, first = int(n_body), int(first)
    _check_body(n, num, den, n_body)
    stride = int(stride)
    if stride < 1 or first < 0:
        raise SushiError('resample: the slice lies outside the body')
    count = max(0, (n_body - first + stride - 1) // stride) if count is None else int(count)
    if count < 0 or (count and first + (count - 1) * stride > n_body - 1):
        raise SushiError('resample: the slice lies outside the body')
    if num == den:
        return np.array(x[first + stride * np.arange(count, dtype=np.int64)], dtype=np.float32)
    _, _, W, H = fir_table(fr, sr)
    out = np.empty(count, np.float32)
    for b0 in range(0, count, _HOST_BLOCK):
        i = first + stride * np.arange(b0, min(b0 + _HOST_BLOCK, count), dtype=np.int64)
        t = i * np.int64(num)
        j = t // den
        r = t % den
        lo = j - (W - 1)
        acc = np.zeros(i.shape[0], np.float64)
        for c in range(2 * W):
            h = H[0, c] if den == 1 else H[r, c]
            p = h * x[np.clip(lo + c, 0, n - 1)].astype(np.float64)
            acc = acc + p
        out[b0:b0 + i.shape[0]] = acc.astype(np.float32)
    return out


def resample_device(tensor, fr, sr, n_body, pad=0, total=None, out=None):
    """One call of sushi_hip_load_resample_fir on a contiguous 1-D float32 CUDA tensor of frames at rate `fr`: uploads the table
    and filters.  Returns the float32 row of `total` samples (default 2 * pad + n_body): the body at [pad, pad + n_body), zeros from
    there to total - pad, both pads filled with the neighbouring inner sample -- the layout of the nearest path's row.  out: a
    contiguous 1-D float32 CUDA tensor of `total` samples to write instead.  fr == sr: no table, the body is a copy.
    Asynchronous on the current torch stream of the tensor's device (the table's upload is ordered on it too)."""
    import torch
    from .device import _raw_stream
    if not isinstance(tensor, torch.Tensor) or tensor.dim() != 1 or not tensor.is_cuda or not tensor.is_contiguous() or \
            tensor.dtype != torch.float32:
        raise SushiError('resample: a contiguous 1-D float32 CUDA tensor')
    n = int(tensor.shape[0])
    num, den = ratio(fr, sr)
    n_body, pad = int(n_body), int(pad)
    _check_body(n, num, den, n_body)
    total = 2 * pad + n_body if total is None else int(total)
    if pad < 0 or pad + n_body > total - pad:
        raise SushiError('resample: the body does not fit between the pads')
    dev = tensor.device
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(total, dtype=torch.float32, device=dev)
        elif not isinstance(out, torch.Tensor) or out.dim() != 1 or out.dtype != torch.float32 or out.device != dev or \
                not out.is_contiguous() or int(out.shape[0]) != total:
            raise SushiError('resample: out must be a contiguous 1-D float32 CUDA tensor of `total` samples on the input\'s device')
        if num == den:
            out[pad:pad + n_body] = tensor[:n_body]
            out[pad + n_body:total - pad] = 0
            fill_pads(out, pad)
            return out
        _, _, W, H = fir_table(fr, sr)
        table = torch.from_numpy(np.array(H)).to(dev)          # (a pageable upload: the bytes have left the host when it returns)
        rc = _native.lib().sushi_hip_load_resample_fir(tensor.data_ptr(), n, num, den, table.data_ptr(), W, n_body, pad, total,
                                                       out.data_ptr(), _raw_stream(dev))
        _native.check(rc, "sushi_hip_load_resample_fir")
    return out
