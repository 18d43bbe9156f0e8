"""A source that plays at another speed than the destination (PAL / NTSC: 25/24, 1001/960, 1001/1000 and their inverses).

``speed`` means everywhere: how fast the SOURCE plays relative to the destination.  A source instant ``t`` lies at
``t * speed`` on the destination's clock, so retiming a source to that clock reads it at a step of ``1 / speed`` input samples
per output sample: ``num = speed.denominator``, ``den = speed.numerator``.

* ``retime_host`` / ``retime_device`` -- linear interpolation at a rational step in the arithmetic of ``sushi_hip_retime``
  (include/sushi_hip.h): NumPy float64 on the host, one kernel launch on the GPU, bit for bit the same.
* ``estimate_speed`` -- which of a few candidate speeds a source plays at: one retime launch + one batch of searches.
* ``choose_speed`` / ``fit_speed`` -- its decision rule and its fit, pure functions of numbers.
"""
import time
from fractions import Fraction

import numpy as np

from . import _native
from .common import Record, SushiError
from .rowcheck import device_out, device_row, host_row

MAX_TERM = 1 << 20           # numerator and denominator of a step (sushi_hip_retime)
MAX_RATIO = 8                # a step lies in [1/8, 8]
STANDARD_SPEEDS = (Fraction(1), Fraction(25, 24), Fraction(24, 25), Fraction(1001, 960), Fraction(960, 1001),
                   Fraction(1001, 1000), Fraction(1000, 1001))
AMBIGUITY = 0.25             # the best candidate's median score must be at most this times the runner-up's


def as_ratio(speed):
    """A speed as a fractions.Fraction: a Fraction, an int, a "25/24" string, or a float (through
    Fraction(x).limit_denominator(100000)).  SushiError if numerator or denominator exceeds 2^20 or the ratio lies outside [1/8, 8]."""
    if isinstance(speed, bool):
        raise SushiError("speed must be a number or a 'p/q' string")
    try:
        if isinstance(speed, (Fraction, int, np.integer)):
            f = Fraction(int(speed)) if not isinstance(speed, Fraction) else speed
        elif isinstance(speed, str):
            f = Fraction(speed.strip().replace(" ", ""))
        elif isinstance(speed, (float, np.floating)):
            f = Fraction(float(speed)).limit_denominator(100000)
        else:
            raise SushiError("speed must be a Fraction, an int, a float or a 'p/q' string")
    except (ValueError, ZeroDivisionError, OverflowError) as e:
        raise SushiError("not a speed: %r (%s)" % (speed, e))
    if f <= 0 or f.numerator > MAX_TERM or f.denominator > MAX_TERM:
        raise SushiError("speed %s: numerator and denominator must lie in 1..2^20" % f)
    if f > MAX_RATIO or f < Fraction(1, MAX_RATIO):
        raise SushiError("speed %s lies outside [1/8, 8]" % f)
    return f


def speed_segment(speed, in_start, out_off, out_len):
    """The segment (in_start, out_off, out_len, num, den) that puts source samples from in_start on onto the destination's clock."""
    s = as_ratio(speed)
    return (int(in_start), int(out_off), int(out_len), s.denominator, s.numerator)


def _segments(segments, n_in, n_out=None):
    """Segments (a RETIME_SEGMENT_DTYPE array, or an iterable of (in_start, out_off, out_len, num, den)) as that array, after the
    checks of sushi_hip_retime; returns (array, smallest output length that holds them)."""
    if isinstance(segments, np.ndarray) and segments.dtype == _native.RETIME_SEGMENT_DTYPE:
        seg = np.ascontiguousarray(segments).reshape(-1)
    else:
        rows = [tuple(int(v) for v in s) for s in segments]
        if any(len(r) != 5 for r in rows):
            raise SushiError("a segment is (in_start, out_off, out_len, num, den)")
        if any(not (0 < r[3] <= MAX_TERM and 0 < r[4] <= MAX_TERM) for r in rows):
            raise SushiError("a step's numerator and denominator must lie in 1..2^20")
        seg = np.array(rows, dtype=_native.RETIME_SEGMENT_DTYPE).reshape(-1)
    if seg.shape[0] < 1:
        raise SushiError("no segments")
    num, den = seg["num"].astype(np.int64), seg["den"].astype(np.int64)
    if (num < 1).any() or (num > MAX_TERM).any() or (den < 1).any() or (den > MAX_TERM).any():
        raise SushiError("a step's numerator and denominator must lie in 1..2^20")
    if (num > MAX_RATIO * den).any() or (den > MAX_RATIO * num).any():
        raise SushiError("a step must lie in [1/8, 8]")
    if (seg["out_len"] < 1).any() or (seg["out_len"] >= 1 << 40).any():
        raise SushiError("a segment has 1 .. 2^40 - 1 outputs")
    if (seg["in_start"] < 0).any() or (seg["in_start"] > n_in - 1).any() or \
            ((seg["out_len"] - 1) * num // den > n_in - 1 - seg["in_start"]).any():
        raise SushiError("a segment reads outside its input")
    need = int((seg["out_off"] + seg["out_len"]).max())
    if (seg["out_off"] < 0).any() or (n_out is not None and need > n_out):
        raise SushiError("a segment writes outside its output")
    return seg, need


_HOST_BLOCK = 1 << 22        # outputs per NumPy pass of retime_host (bounds its temporaries)


def retime_host(samples, segments, out=None):
    """sushi_hip_retime in NumPy (include/sushi_hip.h states the arithmetic), and the CPU path: for output i of a segment
    t = i * num (int64), j = in_start + t // den, r = t % den, j1 = min(j + 1, n - 1), w = r / den (float64),
    y = x[j] + w * (x[j1] - x[j]) in float64; float32 output (float32)y, uint8 output (uint8)(y + 0.5).
    samples: a 1-D uint8 / float32 array; segments: (in_start, out_off, out_len, num, den) each.  out: an array of that dtype to
    write into (samples outside every segment keep their value); None: zeros of the smallest length that holds the segments."""
    x = host_row("retime", samples)
    n = x.shape[0]
    seg, need = _segments(segments, n, None if out is None else out.shape[0])
    if out is None:
        out = np.zeros(need, x.dtype)
    elif out.ndim != 1 or out.dtype != x.dtype:
        raise SushiError("retime: out must be a 1-D array of the samples' dtype")
    for s in seg:
        in_start, out_off, out_len, num, den = (int(s[k]) for k in ("in_start", "out_off", "out_len", "num", "den"))
        for b0 in range(0, out_len, _HOST_BLOCK):
            i = np.arange(b0, min(b0 + _HOST_BLOCK, out_len), dtype=np.int64)
            t = i * np.int64(num)
            j = in_start + t // den
            r = t % den
            j1 = np.minimum(j + 1, n - 1)
            a = x[j].astype(np.float64)
            d = x[j1].astype(np.float64) - a
            w = r.astype(np.float64) / np.float64(den)
            p = w * d
            y = a + p
            dst = out[out_off + b0:out_off + b0 + i.shape[0]]
            if x.dtype == np.uint8:
                dst[:] = (y + 0.5).astype(np.uint8)
            else:
                dst[:] = y.astype(np.float32)
    return out


def retime_device(tensor, segments, out=None, hip_stream=None):
    """One call of sushi_hip_retime on a contiguous 1-D uint8 / float32 CUDA tensor.  out: a contiguous 1-D CUDA tensor of the same
    dtype and device to write into (samples outside every segment keep their value); None: a new one of the smallest length that
    holds the segments, zero outside them.  Asynchronous on hip_stream (default: the current torch stream of the tensor's device)."""
    import torch
    from .device import _launch
    code = device_row("retime", tensor)
    n = int(tensor.shape[0])
    seg, need = _segments(segments, n, None if out is None else int(out.shape[0]))
    L = _native.lib()
    dev = tensor.device
    if out is None:
        out = torch.zeros(need, dtype=tensor.dtype, device=dev)
    else:
        device_out("retime", tensor, out)
    _launch("sushi_hip_retime", dev, L.sushi_hip_retime_bytes(seg.shape[0]),
            lambda mem, mem_bytes, st: L.sushi_hip_retime(tensor.data_ptr(), code, n, seg.ctypes.data, seg.shape[0],
                                                          out.data_ptr(), int(out.shape[0]), mem, mem_bytes, st),
            (tensor, out), hip_stream)
    return out


# ---------------------------------------------------------------------------------------------- which speed is it?
def choose_speed(candidates, score_matrix):
    """The decision of estimate_speed: score_matrix[c][p] is probe p's best TM_SQDIFF_NORMED score with the pattern retimed by
    candidate c (NaN: no such probe).  Returns (speed, scores): scores[c] the median over the probes, speed the candidate with the
    lowest median -- or None (ambiguous) unless that median is at most 0.25 x the second-lowest (or there is no second candidate
    to hold it against)."""
    cands = [as_ratio(c) for c in candidates]
    m = np.asarray(score_matrix, dtype=np.float64).reshape(len(cands), -1)
    if m.shape[1] < 1 or np.isnan(m).all(axis=1).any():
        raise SushiError("choose_speed: every candidate needs at least one probe score")
    scores = np.nanmedian(m, axis=1)
    order = np.argsort(scores, kind="stable")
    if len(cands) < 2 or not scores[order[0]] <= AMBIGUITY * scores[order[1]]:
        return None, scores
    return cands[int(order[0])], scores


def fit_speed(src_index, dst_index):
    """Theil-Sen slope of destination index over source index: the median of the slopes of all pairs of points (robust against a
    probe that matched in the wrong place)."""
    s = np.asarray(src_index, dtype=np.float64).reshape(-1)
    d = np.asarray(dst_index, dtype=np.float64).reshape(-1)
    if s.shape[0] != d.shape[0]:
        raise SushiError("fit_speed: equally many source and destination indices")
    a, b = np.triu_indices(s.shape[0], 1)
    keep = s[a] != s[b]
    if not keep.any():
        raise SushiError("fit_speed: needs two probes at different source positions")
    return float(np.median((d[b][keep] - d[a][keep]) / (s[b][keep] - s[a][keep])))


class SpeedEstimate(Record):
    """What estimate_speed found.
    candidates    the speeds tried (Fractions);
    scores        the median probe score per candidate;
    speed         the candidate with the lowest median, or None: ambiguous (choose_speed);
    best          that candidate whether or not it was accepted;
    fitted        Theil-Sen slope of found destination index over source index, from `best`'s probes -- what the matches themselves say
                  the speed is (None with fewer than two probes);
    offset_seconds  median over `best`'s probes of dst_index / sample_rate - best * src_time;
    probe_scores  [candidate][probe] scores;  probe_src_index / probe_dst_index: where `best`'s probes start in the source body and
                  were found in the destination body (samples);
    seconds       wall time of the call."""

    def __repr__(self):
        return "SpeedEstimate(speed=%s, fitted=%r, offset_seconds=%r, scores=%s)" % (
            self.speed, self.fitted, self.offset_seconds, np.array2string(np.asarray(self.scores), precision=4))


def probe_starts(data_row, padding_size, sample_count, sample_rate, probes, probe_len):
    """First samples (row indices) of estimate_speed's probes: evenly spaced starts between 10 % and 90 % of the body; a slice whose
    samples are all equal is replaced by the next non-flat one one second later (given up after 10 tries: that probe is dropped)."""
    body = int(sample_count)
    if probe_len < 2 or probe_len > body:
        raise SushiError("estimate_speed: probes longer than the source")
    last = padding_size + body - probe_len
    out = []
    for k in range(probes):
        frac = 0.5 if probes == 1 else 0.1 + 0.8 * k / (probes - 1)
        s = min(padding_size + int(body * frac), last)
        for _ in range(10):
            if s > last:
                break
            sl = data_row[s:s + probe_len]
            if (sl != sl[0]).any():
                out.append(s)
                break
            s += int(sample_rate)
    return out


def estimate_speed(src, dst, candidates=STANDARD_SPEEDS, probes=8, probe_seconds=3.0):
    """Which of `candidates` is the speed the WavStream `src` plays at relative to the WavStream `dst` (same sample rate and type)?
    `probes` slices of `probe_seconds` are taken from the source; every one is retimed by every candidate (one sushi_hip_retime
    launch into one pattern pool) and searched in the whole destination row (one FFT-path batch of len(candidates) * probes
    TM_SQDIFF_NORMED searches).  Returns a SpeedEstimate; its `speed` is None where no candidate stands out (choose_speed).
    A true speed that is not among the candidates is out of scope: no candidate then stands out, or a near one does with a poor
    score -- `fitted` (the slope the matches themselves show) tells the caller what to try next.  Needs a GPU."""
    import torch
    from .device import DeviceStream, SearchBatch
    t0 = time.perf_counter()
    cands = [as_ratio(c) for c in candidates]
    if not cands or int(probes) < 1:
        raise SushiError("estimate_speed: needs candidates and probes")
    if src.sample_rate != dst.sample_rate or src.data.dtype != dst.data.dtype:
        raise SushiError("estimate_speed: source and destination must share sample rate and sample type")
    rate = src.sample_rate
    probe_len = int(probe_seconds * rate)
    starts = probe_starts(src.data[0], src.padding_size, src.sample_count, rate, int(probes), probe_len)
    if not starts:
        raise SushiError("estimate_speed: the source is flat wherever it was probed")
    segs, offs, lens = [], [], []
    pool_len = 0
    for c in cands:
        for s in starts:
            m = int(probe_len * c)
            segs.append(speed_segment(c, s, pool_len, m))
            offs.append(pool_len)
            lens.append(m)
            pool_len += m
    dst_dev = dst.device_stream()
    src_row = src.device_stream().raw
    if src_row.device != dst_dev.device:
        raise SushiError("estimate_speed: source and destination live on different devices")
    pool = retime_device(src_row, segs, out=torch.empty(pool_len, dtype=src_row.dtype, device=src_row.device))
    pool_dev = DeviceStream(pool)
    n_dst = dst.data.shape[1]
    if max(lens) > n_dst:
        raise SushiError("estimate_speed: probes longer than the destination")
    batch = SearchBatch(dst_dev, pool_dev, offs, lens, [0] * len(lens), [n_dst - m + 1 for m in lens], path="fft",
                        method="sqdiff_normed")
    batch.run()
    idx, score = batch.results()
    shape = (len(cands), len(starts))
    probe_scores = np.asarray(score, np.float64).reshape(shape)
    found = np.asarray(idx, np.int64).reshape(shape)
    speed, scores = choose_speed(cands, probe_scores)
    best_at = int(np.argmin(scores))
    best = cands[best_at]
    src_index = np.asarray(starts, np.int64) - int(src.padding_size)
    dst_index = found[best_at] - int(dst.padding_size)
    fitted = fit_speed(src_index, dst_index) if len(starts) >= 2 else None
    offset = float(np.median(dst_index / float(rate) - float(best) * (src_index / float(rate))))
    return SpeedEstimate(candidates=cands, scores=scores, speed=speed, best=best, fitted=fitted, offset_seconds=offset,
                         probe_scores=probe_scores, probe_src_index=src_index, probe_dst_index=dst_index,
                         seconds=time.perf_counter() - t0)
