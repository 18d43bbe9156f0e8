"""A slow drift: score rows searched along a line of shifts.

A joint search (sushi_amd.joint) assumes the events of a group share one constant shift.  Two releases of one programme often
differ by a small, unlisted rate -- two captures on different clocks, a residual after a speed correction -- and the shift then
moves along the programme.  Here every event's exact score row (``sushi_hip_match_curves``) is put on one shift axis, and for every
candidate rate r and displacement k the rows are summed along the sloped line k + round(r * (pos_e - anchor)); the answer is the
first extremum over all (rate, displacement) pairs (include/sushi_hip.h "drift search").  No lone decision is made.

* ``drift_host`` -- the arithmetic in NumPy float64, bit for bit what the kernel gives; the CPU path of the reduction.
* ``drift_reduce_device`` -- one call of ``sushi_hip_drift_reduce`` on a buffer of curves.
* ``rate_grid`` / ``drift_anchor`` / ``drift_offsets`` -- candidate rates and the offset table they give: pure functions of numbers.
* ``find_drift`` -- what ``WavStream.find_drift`` runs: one ``match_curves`` call, one drift call, one joint call for the events'
  lone extrema.
"""
from collections import namedtuple
import math

import numpy as np

from . import _native, axis
from .common import Record, SushiError
from .joint import MAX_BYTES, joint_reduce_device

MAX_DRIFTS = 65535           # candidates of one sushi_hip_drift_reduce call

DriftHost = namedtuple("DriftHost", "drift index score row_scores drift_index drift_scores lines")
DriftDevice = namedtuple("DriftDevice", "best score row_scores drift_index drift_scores lines")


def checked_offsets(offsets, n_rows, n_shift):
    """`offsets` as a C-contiguous int32 array [n_drifts][n_rows] after the checks of sushi_hip_drift_reduce, and every candidate's
    valid range: (offsets, lo, hi), lo = max(0, max_e -o), hi = n_shift - max(0, max_e o) (int64 arrays)."""
    o = np.asarray(offsets)
    if o.ndim != 2 or o.shape[1] != n_rows or not np.issubdtype(o.dtype, np.integer):
        raise SushiError("drift: offsets are integers [n_drifts][n_rows]")
    if not 1 <= o.shape[0] <= MAX_DRIFTS:
        raise SushiError("drift: 1 .. %d candidates, not %d" % (MAX_DRIFTS, o.shape[0]))
    wide = o.astype(np.int64)
    if (wide < -2 ** 31).any() or (wide > 2 ** 31 - 1).any():
        raise SushiError("drift: offsets are int32")
    lo = np.maximum(0, (-wide).max(axis=1))
    hi = int(n_shift) - np.maximum(0, wide.max(axis=1))
    if (hi <= lo).any():
        d = int(np.argmax(hi <= lo))
        raise SushiError("drift: candidate %d has no index at which every row is addressed inside its %d shifts" % (d, n_shift))
    return np.ascontiguousarray(wide.astype(np.int32)), lo, hi


def drift_host(rows, weights, offsets, method="sqdiff_normed"):
    """sushi_hip_drift_reduce in NumPy (include/sushi_hip.h states the arithmetic): rows, a list of E >= 1 float32 arrays of one
    length n_shift >= 1; weights, E finite float64 values >= 0; offsets, integers [D][E], D in 1 .. 65535.  Candidate d is valid on
    [lo_d, hi_d) = [max(0, max_e -o), n_shift - max(0, max_e o)) (SushiError if that is empty); there acc = 0.0; acc = acc + w_e *
    float64(R_e[j + o[d][e]]) row after row; line[d][j] = float32(acc).  Returns a DriftHost: drift, index (the first candidate in
    table order, then the first index, of the best value: minimum for 'sqdiff_normed', maximum for 'ccoeff_normed'), score
    (float32), row_scores (R_e[index + o[drift][e]]), drift_index / drift_scores (every candidate's own first extremum over its
    range), lines (float32 [D][n_shift]; +inf / -inf outside a candidate's range)."""
    axis.method_code(method)
    rows = list(rows)
    w = axis.checked_weights(weights, len(rows), "drift")
    rows = axis.checked_score_rows(rows, "drift")
    n = rows[0].shape[0]
    o, lo, hi = checked_offsets(offsets, len(rows), n)
    D = o.shape[0]
    lines = np.full((D, n), -np.inf if method == "ccoeff_normed" else np.inf, np.float32)
    drift_index = np.empty(D, np.int32)
    for d in range(D):
        a, b = int(lo[d]), int(hi[d])
        acc = np.zeros(b - a, np.float64)
        for r, wi, oe in zip(rows, w, o[d]):
            p = wi * r[a + int(oe):b + int(oe)].astype(np.float64)
            acc = acc + p
        lines[d, a:b] = acc.astype(np.float32)
        drift_index[d] = a + axis.first_extremum(lines[d, a:b], method)
    drift_scores = lines[np.arange(D), drift_index]
    best = axis.first_extremum(drift_scores, method)
    index = int(drift_index[best])
    return DriftHost(best, index, drift_scores[best], np.array([r[index + int(oe)] for r, oe in zip(rows, o[best])], np.float32),
                     drift_index, drift_scores, lines)


def drift_reduce_device(curves, rows, n_shift, offsets, method="sqdiff_normed", with_lines=False, hip_stream=None):
    """One call of sushi_hip_drift_reduce on `curves`, a contiguous 1-D float32 CUDA tensor (match_curves' output).  rows:
    (curve_off, weight) each, every row n_shift floats; offsets: integers [n_drifts][n_rows].  Returns a DriftDevice of CUDA
    tensors: best int32[2] (candidate, index), score float32[1], row_scores float32[n_rows], drift_index int32[n_drifts],
    drift_scores float32[n_drifts], lines (with_lines: float32 [n_drifts][n_shift]; else None).  Asynchronous on hip_stream
    (default: the current torch stream of the tensor's device)."""
    import torch
    from .device import _launch
    code = axis.method_code(method)
    axis.check_curves(curves, "drift")
    rt = axis.row_table(rows)
    n_rows, n_shift = rt.shape[0], int(n_shift)
    if n_rows < 1 or not 1 <= n_shift <= 2 ** 31 - 1:
        raise SushiError("drift: >= 1 rows of 1 .. 2^31 - 1 shifts")
    axis.check_rows_inside(rt, int(curves.numel()), n_shift, "drift")
    axis.checked_weights(rt["weight"], n_rows, "drift")
    o, _lo, _hi = checked_offsets(offsets, n_rows, n_shift)
    n_drifts = o.shape[0]
    L = _native.lib()
    dev = curves.device
    best = torch.empty(2, dtype=torch.int32, device=dev)
    score = torch.empty(1, dtype=torch.float32, device=dev)
    row_score = torch.empty(n_rows, dtype=torch.float32, device=dev)
    drift_idx = torch.empty(n_drifts, dtype=torch.int32, device=dev)
    drift_score = torch.empty(n_drifts, dtype=torch.float32, device=dev)
    lines = torch.empty((n_drifts, n_shift), dtype=torch.float32, device=dev) if with_lines else None
    _launch("sushi_hip_drift_reduce", dev, L.sushi_hip_drift_bytes(n_rows, n_drifts),
            lambda mem, mem_bytes, st: L.sushi_hip_drift_reduce(
                curves.data_ptr(), int(curves.numel()), rt.ctypes.data, n_rows, n_shift, o.ctypes.data, n_drifts, code, mem,
                mem_bytes, best.data_ptr(), score.data_ptr(), row_score.data_ptr(), drift_idx.data_ptr(), drift_score.data_ptr(),
                None if lines is None else lines.data_ptr(), st),
            (curves, best, score, row_score, drift_idx, drift_score, lines), hip_stream)
    return DriftDevice(best, score, row_score, drift_idx, drift_score, lines)


# ---------------------------------------------------------------------------------------------- rates -> offsets: numbers only
def rate_grid(max_rate, half_span, resolution=1.0, max_drifts=16384):
    """Candidate rates for events that lie up to half_span samples from the anchor: H = ceil(max_rate * half_span / resolution),
    rates[d] = (d - H) * (resolution / half_span) for d = 0 .. 2 H, ascending, with an exact 0 in the middle: one step moves the
    farthest event by `resolution` samples, and the grid reaches at least +-max_rate.  half_span 0 (one position) gives [0.0].
    SushiError naming the number of candidates when it is above max_drifts."""
    max_rate, half_span, resolution = float(max_rate), float(half_span), float(resolution)
    if not (math.isfinite(max_rate) and max_rate >= 0 and math.isfinite(half_span) and half_span >= 0 and
            math.isfinite(resolution) and resolution > 0):
        raise SushiError("rate_grid: max_rate >= 0, half_span >= 0, resolution > 0, all finite")
    if half_span == 0:
        return np.zeros(1, np.float64)
    H = int(math.ceil(max_rate * half_span / resolution))
    if 2 * H + 1 > int(max_drifts):
        raise SushiError("rate_grid: max_rate %g over a half span of %g samples at a resolution of %g samples is D = %d candidates, "
                         "max_drifts is %d" % (max_rate, half_span, resolution, 2 * H + 1, int(max_drifts)))
    return (np.arange(2 * H + 1, dtype=np.int64) - H).astype(np.float64) * (resolution / half_span)


def drift_anchor(positions):
    """(min + max) // 2 of the integer positions: where a candidate's offset is zero."""
    p = [int(x) for x in positions]
    if not p:
        raise SushiError("drift: no positions")
    return (min(p) + max(p)) // 2


def drift_offsets(positions, rates, anchor=None):
    """o[d][e] = int(np.rint(rates[d] * float(positions[e] - anchor))), an int32 array [len(rates)][len(positions)]; anchor:
    drift_anchor(positions) when not given.  SushiError for an offset that does not fit int32."""
    anchor = drift_anchor(positions) if anchor is None else int(anchor)
    rel = np.array([float(int(p) - anchor) for p in positions], np.float64)
    r = np.asarray(rates, np.float64).reshape(-1)
    if rel.shape[0] < 1 or r.shape[0] < 1 or not np.isfinite(r).all():
        raise SushiError("drift_offsets: >= 1 positions and >= 1 finite rates")
    o = np.rint(r[:, None] * rel[None, :])
    if (np.abs(o) > 2 ** 31 - 1).any():
        raise SushiError("drift_offsets: an offset does not fit int32")
    return o.astype(np.int32)


# ---------------------------------------------------------------------------------------------- WavStream.find_drift
class DriftMatch(Record):
    """What a drift search found.
    rate             seconds of shift per second of programme (= samples per sample): event i is found at
                     window_centers[i] + delta + rate * (window_centers[i] - anchor), rounded to a sample (event_deltas);
    anchor           the instant (seconds, on the window centres' clock) at which the shift is delta;  delta: the shift there;
    score            the line's score (float32);  index: its index on the shift axis (k = k_lo + index);  drift: the candidate;
    k_lo, n_shift    the shift axis: displacements k_lo .. k_lo + n_shift - 1 samples (joint_window over all events);
    event_deltas     every event's own shift on the line, (k_lo + index + o_e) / sample_rate (seconds, list);
    event_scores     every event's own score there (float32 array);
    event_own_delta  where every event's lone search over the same range lands (seconds, list), event_own_scores its score;
    drift_rates / drift_scores / drift_deltas   the profile over rate: every candidate's rate, best score and shift at the anchor
                     there; its sharpness is the caller's confidence;
    rate_ties        every candidate rate whose best score equals the answer's bit for bit (events clustered near the anchor give
                     candidates the same offsets: the answer is then the lowest such rate);
    lines            float32 [candidates][n_shift] (with_lines=True), or None;
    clamp, rows_info None, or with clamp= the float32 value f the rows were clamped at (as a float) and what forming them took
                     (axis.event_rows' info).  score, the profile over rate, lines and the own extrema are then those of the clamped
                     rows: an event_own_scores entry equal to f with its event_own_delta at index 0 (k_lo) means nothing in that
                     event's window passed.  event_scores stay the true scores on the line, formed one position each."""

    def __repr__(self):
        return "DriftMatch(rate=%r, delta=%r, score=%r, events=%d)" % (self.rate, self.delta, float(self.score), len(self.event_scores))


def find_drift(stream, patterns, window_centers, window_size, max_rate, resolution=1.0, weights="equal", method="sqdiff_normed",
               with_lines=False, max_bytes=MAX_BYTES, clamp=None, capacity=None):
    """WavStream.find_drift (its docstring)."""
    axis.method_code(method)
    f, capacity = axis.checked_clamp(clamp, capacity, method)
    patterns, centres = list(patterns), list(window_centers)
    if not patterns or len(patterns) != len(centres):
        raise SushiError("find_drift: equally many patterns and centres (>= 1)")
    dst_dev = stream.device_stream()
    src_dev, offs, lens, _ = stream._pattern_source(patterns, dst_dev)
    lens = axis.pattern_lengths(lens)
    E = len(patterns)
    w = axis.event_weights(weights, lens, per_event=False)
    ax = axis.event_axis(stream, offs, lens, centres, window_size)
    k_lo, n_shift, hz = ax.k_lo, ax.n_shift, stream.sample_rate
    anchor = drift_anchor(ax.bases)
    half_span = max(max(ax.bases) - anchor, anchor - min(ax.bases))
    rates = rate_grid(max_rate, half_span, resolution)
    offsets = drift_offsets(ax.bases, rates, anchor)
    reach = int((np.maximum(0, offsets.max(axis=1).astype(np.int64)) + np.maximum(0, (-offsets.astype(np.int64)).max(axis=1))).max())
    if reach >= n_shift:
        raise SushiError("find_drift: max_rate %g moves the events %d samples apart, the window leaves %d shifts: window_size must "
                         "be at least the uncertainty of the base shift + max_rate x half span = %g s"
                         % (float(max_rate), reach, n_shift, float(max_rate) * half_span / float(hz)))
    need = 4 * E * n_shift
    if need > max_bytes:
        raise SushiError("find_drift: %d events x %d shifts need %d bytes of curves at once, max_bytes is %d"
                         % (E, n_shift, need, max_bytes))
    info = None if f is None else {}
    curves, row_off = axis.event_rows(dst_dev, src_dev, [ax], method, clamp=f, capacity=capacity, info=info)
    res = drift_reduce_device(curves, zip(row_off, w), n_shift, offsets, method=method, with_lines=with_lines)
    own = joint_reduce_device(curves, zip(row_off, w), [(0, E, n_shift)], method=method)
    best, score, row_score, drift_idx, drift_score = (t.cpu().numpy() for t in res[:5])
    d, j = int(best[0]), int(best[1])
    if f is not None:
        # every event's true score on the line: the rows hold f where nothing passes, so one position each is formed
        from .curves import match_curves
        row_score = match_curves(dst_dev, src_dev, ax.offs, lens, [b + k_lo + j + int(o) for b, o in zip(ax.bases, offsets[d])],
                                 [1] * E, method=method)[0].cpu().numpy()
    ties = np.flatnonzero(drift_score.view(np.uint32) == drift_score.view(np.uint32)[d])
    return DriftMatch(
        rate=float(rates[d]), anchor=(anchor - stream.padding_size) / float(hz), delta=(k_lo + j) / float(hz), score=score[0],
        index=j, drift=d, k_lo=k_lo, n_shift=n_shift,
        event_deltas=[(k_lo + j + int(o)) / float(hz) for o in offsets[d]], event_scores=row_score,
        event_own_delta=[(k_lo + int(k)) / float(hz) for k in own.row_own_index.cpu().numpy()],
        event_own_scores=own.row_own_scores.cpu().numpy(),
        drift_rates=rates, drift_scores=drift_score, drift_deltas=(k_lo + drift_idx.astype(np.int64)) / float(hz),
        rate_ties=[float(rates[t]) for t in ties], lines=res.lines.cpu().numpy() if with_lines else None,
        clamp=None if f is None else float(f), rows_info=None if info is None else axis.merge_rows_info(None, info))
