"""Matching on loudness contours: two releases of one programme whose waveforms differ -- inverted polarity, a
speed change with the pitch kept, another carrier under the same contour -- still share the mean absolute deviation over a few
milliseconds.

* ``envelope_host`` / ``envelope_device`` -- a row's contour in the arithmetic of ``sushi_hip_envelope`` (include/sushi_hip.h):
  NumPy on the host, one kernel launch on the GPU, bit for bit the same.  ``WavStream.envelope`` makes a live stream of it.
* ``find_coarse_fine`` -- a two-stage search: every event on the contours over a wide window, then on the waveforms in a narrow
  window around the contour's answer.  It reports both and decides nothing.
"""
import time

import numpy as np

from . import _native
from .common import Record, SushiError
from .rowcheck import device_out, device_row, host_row, row_span

MAX_HOP, MAX_SPAN, MAX_WINDOW = 256, 64, 4096        # hop, span, hop * span (sushi_hip_envelope)

_HOST_SAMPLES = 1 << 22      # input samples gathered per NumPy pass of envelope_host (bounds its temporaries)


def _check(n_in, in_start, hop, span, out_len):
    """The checks of sushi_hip_envelope on Python integers; returns them as ints."""
    in_start, hop, span, out_len = int(in_start), int(hop), int(span), int(out_len)
    if not 1 <= hop <= MAX_HOP or not 1 <= span <= MAX_SPAN or hop * span > MAX_WINDOW:
        raise SushiError("envelope: hop in 1..256, span in 1..64, hop * span <= 4096")
    row_span("envelope", n_in, in_start, out_len)
    return in_start, hop, span, out_len


def envelope_host(samples, in_start, hop, span, out_len):
    """sushi_hip_envelope in NumPy (include/sushi_hip.h states the arithmetic), and the CPU path.  With a = (span - 1) // 2,
    W = hop * span and c the sample type's centre (128 / 0.5): block sum B_b = sum over t = 0 .. hop - 1, in that order, of
    |x[clip(in_start + b * hop + t, 0, n - 1)] - c|; output i sums B_{i-a} .. B_{i-a+span-1} in that order to E.  uint8: integers,
    min(255, (4 E + W) // (2 W)); float32: float64 running sums from 0.0 (one rounding per addition), (float32)((E + E) / W).
    samples: a 1-D uint8 / float32 array.  Returns out_len samples of its dtype."""
    x = host_row("envelope", samples)
    n = x.shape[0]
    in_start, hop, span, out_len = _check(n, in_start, hop, span, out_len)
    a, w = (span - 1) // 2, hop * span
    u8 = x.dtype == np.uint8
    out = np.empty(out_len, x.dtype)
    step = max(1, _HOST_SAMPLES // hop)
    t = np.arange(hop, dtype=np.int64)
    for i0 in range(0, out_len, step):
        n_out = min(step, out_len - i0)
        blocks = np.arange(i0 - a, i0 - a + n_out + span - 1, dtype=np.int64)
        idx = np.clip(in_start + blocks[:, None] * hop + t[None, :], 0, n - 1)
        if u8:
            b = np.abs(x[idx].astype(np.int64) - 128).sum(axis=1)
            e = np.zeros(n_out, np.int64)
        else:
            d = np.abs(x[idx].astype(np.float64) - 0.5)
            b = np.zeros(blocks.shape[0], np.float64)
            for k in range(hop):                          # sequential in t: the kernel's order
                b = b + d[:, k]
            e = np.zeros(n_out, np.float64)
        for j in range(span):                             # ... and in j
            e = e + b[j:j + n_out]
        if u8:
            out[i0:i0 + n_out] = np.minimum((4 * e + w) // (2 * w), 255).astype(np.uint8)
        else:
            out[i0:i0 + n_out] = ((e + e) / np.float64(w)).astype(np.float32)
    return out


def envelope_device(tensor, in_start, hop, span, out_len, out=None, hip_stream=None):
    """One call of sushi_hip_envelope on a contiguous 1-D uint8 / float32 CUDA tensor.  out: a contiguous 1-D CUDA tensor (or
    view) of the same dtype and device with out_len samples to write into; None: a new one.  Asynchronous on hip_stream (default:
    the current torch stream of the tensor's device)."""
    import torch
    from .device import _launch
    code = device_row("envelope", tensor)
    n = int(tensor.shape[0])
    in_start, hop, span, out_len = _check(n, in_start, hop, span, out_len)
    L = _native.lib()
    dev = tensor.device
    if out is None:
        out = torch.empty(out_len, dtype=tensor.dtype, device=dev)
    else:
        device_out("envelope", tensor, out, out_len)
    _launch("sushi_hip_envelope", dev, None,
            lambda mem, mem_bytes, st: L.sushi_hip_envelope(tensor.data_ptr(), code, n, in_start, hop, span,
                                                            out.data_ptr(), out_len, st),
            (tensor, out), hip_stream)
    return out


def envelope_layout(sample_rate, padding_size, sample_count, hop):
    """(sample_rate, padding_size, sample_count) of WavStream.envelope's result: rate // hop (SushiError unless hop divides the
    rate), pad // hop, ceil(count / hop)."""
    hop = int(hop)
    if hop < 1 or int(sample_rate) % hop:
        raise SushiError("envelope: hop %d does not divide the sample rate %d" % (hop, int(sample_rate)))
    return int(sample_rate) // hop, int(padding_size) // hop, (int(sample_count) + hop - 1) // hop


# ---------------------------------------------------------------------------------------------- contour first, waveform second
class CoarseFine(Record):
    """What find_coarse_fine found, one entry per event.
    coarse_shift   seconds by which the contour search moves the event (a multiple of hop / rate);
    coarse_score   its TM_CCOEFF_NORMED value on the contours;
    fine_shift     seconds by which the waveform search around event start + coarse_shift moves the event;
    fine_score     its TM_CCOEFF_NORMED value on the waveforms -- at chance level where the waveforms really differ (inverted
                   polarity: strongly negative at the true place, so the arg-max lies elsewhere): the coarse shift is then the answer;
    coarse_samples / fine_samples   the two shifts in contour samples and in samples (int64);
    hop, span, fine_window;  seconds: wall time of the call."""

    def __repr__(self):
        return "CoarseFine(%d events, hop=%d, span=%d, %.3f s)" % (len(self.coarse_shift), self.hop, self.span, self.seconds)


def _starts(stream, events):
    """Where get_substream starts each event's pattern in the stream's body (samples)."""
    return np.array([stream._get_sample_for_time(s) - stream.padding_size for s, _e in events], np.int64)


def find_coarse_fine(src, dst, events, window, hop=8, span=4, fine_window=None, src_env=None, dst_env=None):
    """Every event (start, end: seconds in the WavStream `src`) looked for in the WavStream `dst` in two stages.  Coarse: one
    dst_env.find_substreams batch with method='ccoeff_normed' on the contours (src_env / dst_env: src.envelope(hop, span) /
    dst.envelope(hop, span), made here unless given -- give them to make them once per job) over +-window seconds around the
    event's own time.  Fine: one dst.find_substreams batch with method='ccoeff_normed' on the waveforms, centred on the event's
    time plus its coarse shift, +-fine_window seconds (default (span + 2) * hop / rate: the contour's own resolution).  Returns a
    CoarseFine with both answers for every event; no decision between them is made.  Needs a GPU."""
    t0 = time.perf_counter()
    events = [(float(s), float(e)) for s, e in events]
    if not events:
        raise SushiError("find_coarse_fine: no events")
    if src.sample_rate != dst.sample_rate or src.data.dtype != dst.data.dtype:
        raise SushiError("find_coarse_fine: source and destination must share sample rate and sample type")
    if src_env is None:
        src_env = src.envelope(hop, span)
    if dst_env is None:
        dst_env = dst.envelope(hop, span)
    rate = src.sample_rate
    env_rate = envelope_layout(rate, 0, 1, hop)[0]
    if src_env.sample_rate != env_rate or dst_env.sample_rate != env_rate:
        raise SushiError("find_coarse_fine: the enveloped streams' rate is not rate // hop")
    if fine_window is None:
        fine_window = (span + 2) * hop / float(rate)
    n = len(events)
    pats = [src_env.get_substream(s, e) for s, e in events]
    if any(p.shape[1] < 1 for p in pats):
        raise SushiError("find_coarse_fine: an event has no samples in the source's contour")
    coarse_score, _times, pos = dst_env.find_substreams(pats, [s for s, _e in events], [window] * n, with_index=True,
                                                       method="ccoeff_normed")
    coarse_samples = np.asarray(pos, np.int64) - int(dst_env.padding_size) - _starts(src_env, events)
    coarse_shift = coarse_samples / float(env_rate)
    pats = [src.get_substream(s, e) for s, e in events]
    if any(p.shape[1] < 1 for p in pats):
        raise SushiError("find_coarse_fine: an event has no samples in the source")
    fine_score, _times, pos = dst.find_substreams(pats, [s + float(c) for (s, _e), c in zip(events, coarse_shift)],
                                                  [fine_window] * n, with_index=True, method="ccoeff_normed")
    fine_samples = np.asarray(pos, np.int64) - int(dst.padding_size) - _starts(src, events)
    return CoarseFine(coarse_shift=coarse_shift, coarse_score=np.asarray(coarse_score, np.float32), coarse_samples=coarse_samples,
                      fine_shift=fine_samples / float(rate), fine_score=np.asarray(fine_score, np.float32),
                      fine_samples=fine_samples, hop=int(hop), span=int(span), fine_window=float(fine_window),
                      seconds=time.perf_counter() - t0)
