"""The shift axis: what the joint search (sushi_amd.joint) and the segmentation pass (sushi_amd.segments) share.  Both lay events'
exact score rows (``sushi_hip_match_curves`` output) on one axis of displacements, weigh them and reduce them (csrc/axis_core.hpp
is the native side of the layer)."""
from collections import namedtuple

import numpy as np

from . import _native
from .common import SushiError


def method_code(method):
    """The library's code of 'sqdiff_normed' / 'ccoeff_normed'; SushiError for anything else."""
    if method not in _native.METHODS:
        raise SushiError("method must be one of %s" % sorted(_native.METHODS))
    return _native.METHODS[method]


def first_extremum(row, method):
    # np.argmin / np.argmax return the first index of the extremum; 0.0 and -0.0 compare equal
    return int(np.argmax(row)) if method == "ccoeff_normed" else int(np.argmin(row))


def checked_weights(weights, n, who):
    """`weights` as a float64 array of n >= 1 finite values >= 0 (who: 'joint' / 'path', for the error)."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if n < 1 or w.shape[0] != n:
        raise SushiError("%s: as many weights as rows (>= 1)" % who)
    if not np.isfinite(w).all() or (w < 0).any():
        raise SushiError("%s: weights must be finite and >= 0" % who)
    return w


def checked_score_rows(rows, who):
    """`rows` as a list of 1-D float32 arrays of one length >= 1: the score rows of a NumPy restatement."""
    rows = [np.asarray(r) for r in rows]
    n = rows[0].shape[0] if rows and rows[0].ndim == 1 else -1
    if n < 1 or any(r.ndim != 1 or r.dtype != np.float32 or r.shape[0] != n for r in rows):
        raise SushiError("%s: rows are 1-D float32 arrays of one length >= 1" % who)
    return rows


def row_table(rows):
    """(curve_off, weight) pairs, or a JOINT_ROW_DTYPE array, as that array (SushiHipJointRow records)."""
    if isinstance(rows, np.ndarray) and rows.dtype == _native.JOINT_ROW_DTYPE:
        return np.ascontiguousarray(rows).reshape(-1)
    return np.array([(int(o), float(w)) for o, w in rows], dtype=_native.JOINT_ROW_DTYPE).reshape(-1)


def check_rows_inside(rt, n_curve, n_shift, who):
    """Every row of the table `rt` stays inside a buffer of n_curve floats (n_shift: a number, or one per row)."""
    if (rt["curve_off"] < 0).any() or (rt["curve_off"] > n_curve - n_shift).any():
        raise SushiError("%s: a row leaves the curve buffer" % who)


def check_curves(curves, who, device=None):
    """`curves` is match_curves' output: a contiguous 1-D float32 CUDA tensor (on `device`, if given)."""
    import torch
    if not isinstance(curves, torch.Tensor) or curves.dim() != 1 or not curves.is_cuda or not curves.is_contiguous() or \
            curves.dtype != torch.float32 or curves.numel() < 1 or (device is not None and curves.device != device):
        raise SushiError("%s: a contiguous 1-D float32 CUDA tensor of curves%s" % (who, "" if device is None else " on the state's device"))


def event_weights(weights, lens, per_event):
    """One weight per event of `lens` samples.  'equal' and 'length' (an event counts by its length M_i) come in two scales: they
    sum to 1 (per_event=False, the joint search: 1 / m and M_i / sum M) or to the number of events (per_event=True, the segmentation
    pass, whose penalty is in units of one event's score: 1.0 and M_i * E / sum M).  A sequence of numbers is taken as it is."""
    m = len(lens)
    if isinstance(weights, str):
        if weights == "equal":
            return [1.0] * m if per_event else [1.0 / m] * m
        if weights == "length":
            total = float(sum(lens))
            return [float(n) * m / total for n in lens] if per_event else [float(n) / total for n in lens]
        raise SushiError("weights: 'equal', 'length' or a sequence of numbers")
    try:
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise SushiError("weights: 'equal', 'length' or a sequence of numbers")
    if len(w) != m:
        raise SushiError("weights: one per event" if per_event else "weights: one per event of the group")
    return w


def joint_window(bases, lens, total, W):
    """Which displacements k every event of a group can take: event i (lens[i] samples) sits at bases[i] + k in a stream of `total`
    samples, |k| <= W.  Returns (k_lo, n_shift): k_lo = max(-W, max_i(-bases[i])), k_hi = min(W, min_i(total - lens[i] - bases[i])),
    n_shift = k_hi - k_lo + 1.  SushiError if no displacement serves every event."""
    bases = [int(b) for b in bases]
    lens = [int(m) for m in lens]
    W = int(W)
    if not bases or len(bases) != len(lens) or W < 0:
        raise SushiError("joint_window: as many lengths as bases (>= 1), W >= 0")
    k_lo = max(-W, max(-b for b in bases))
    k_hi = min(W, min(int(total) - m - b for b, m in zip(bases, lens)))
    if k_hi < k_lo:
        raise SushiError("joint_window: no shift within %d samples keeps every event of the group inside the stream" % W)
    return k_lo, k_hi - k_lo + 1


def pattern_lengths(lens):
    """Located patterns' lengths as ints; SushiError for an empty pattern."""
    lens = [int(m) for m in lens]
    if min(lens) < 1:
        raise SushiError("empty pattern")
    return lens


class EventAxis(namedtuple("EventAxis", "offs lens bases k_lo n_shift")):
    """Events on one shift axis: event i is the pattern of lens[i] samples at offs[i] of the source stream, and sits at sample
    bases[i] + k of the destination for the displacements k = k_lo .. k_lo + n_shift - 1."""
    __slots__ = ()

    def part(self, first, last):
        """Events first .. last - 1, on the same axis."""
        return self._replace(offs=self.offs[first:last], lens=self.lens[first:last], bases=self.bases[first:last])


def event_axis(stream, offs, lens, centres, window_size):
    """The EventAxis of located patterns (offs, lens: WavStream._pattern_source's) looked for around `centres` (seconds) in the
    WavStream `stream`, within window_size seconds (joint_window)."""
    bases = [stream._get_sample_for_time(c) for c in centres]
    k_lo, n_shift = joint_window(bases, lens, int(stream.data.shape[1]), int(stream.sample_rate * window_size))
    return EventAxis([int(o) for o in offs], list(lens), bases, k_lo, n_shift)


def event_curves(dst_dev, src_dev, axes, method):
    """Every event's score row over its axis, for a chunk of EventAxis records: one match_curves call.  Returns (curves, the first
    float of every row in curves, in event order)."""
    from .curves import match_curves
    curves, bounds = match_curves(dst_dev, src_dev, [o for a in axes for o in a.offs], [m for a in axes for m in a.lens],
                                  [b + a.k_lo for a in axes for b in a.bases], [a.n_shift for a in axes for _ in a.bases],
                                  method=method)
    return curves, bounds[:-1].tolist()


# ---------------------------------------------------------------------------------------------- rows clamped at a threshold
HIT_BYTES = 256 << 20        # hit records of one threshold run (event_rows' default capacity stays under it)


def clamp_value(clamp, method):
    """The float32 value f a clamp stands for: the smallest float32 >= clamp for 'sqdiff_normed', the largest float32 <= clamp for
    'ccoeff_normed' -- rounded towards the side that fails, so that a float32 score passes f exactly when it passes `clamp`, and a
    threshold run at float(f) finds exactly the positions a clamped row keeps.  SushiError unless clamp (and f) is finite."""
    code = method_code(method)
    try:
        c = float(clamp)
    except (TypeError, ValueError):
        raise SushiError("clamp must be a number")
    if not np.isfinite(c):
        raise SushiError("clamp must be finite")
    with np.errstate(over="ignore"):
        f = np.float32(c)
    if code == _native.METHOD_CCOEFF_NORMED:
        if float(f) > c:
            f = np.nextafter(f, np.float32(-np.inf))
    elif float(f) < c:
        f = np.nextafter(f, np.float32(np.inf))
    if not np.isfinite(f):
        raise SushiError("clamp must be finite as a float32")
    return np.float32(f)


def clamp_rows_host(rows, clamp, method):
    """The clamped row in NumPy, the statement every other form is compared with: min(R, f) for 'sqdiff_normed' as np.where(R <= f,
    R, f), max(R, f) for 'ccoeff_normed' as np.where(R >= f, R, f), f = clamp_value(clamp, method), the comparison in float64.
    float32, the shape of `rows`; the bits of every passing value are kept, -0.0 included; a NaN becomes f."""
    f = clamp_value(clamp, method)
    R = np.asarray(rows)
    if R.dtype != np.float32:
        raise SushiError("clamp_rows_host: float32 rows")
    wide = R.astype(np.float64)
    keep = wide >= float(f) if method == "ccoeff_normed" else wide <= float(f)
    return np.where(keep, R, f).astype(np.float32)


def checked_clamp(clamp, capacity, method):
    """(f or None, capacity or None) of a search's clamp= / capacity= arguments; SushiError for a capacity without a clamp, or one
    that is not an int >= 0."""
    if clamp is None:
        if capacity is not None:
            raise SushiError("capacity belongs to clamp=")
        return None, None
    f = clamp_value(clamp, method)
    if capacity is not None:
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or capacity < 0:
            raise SushiError("capacity must be an int >= 0")
        capacity = int(capacity)
    return f, capacity


def default_capacity(n_requests, n_shift):
    """Hits kept per request when the caller names none: min(n_shift, max(1024, n_shift // 16)), and no more than HIT_BYTES of
    8-byte records over all requests of the run (at least 1)."""
    return max(1, min(int(n_shift), max(1024, int(n_shift) // 16), HIT_BYTES // (8 * max(1, int(n_requests)))))


def merge_rows_info(total, info):
    """A search's rows_info: event_rows' counts summed over its formings (capacity: the largest)."""
    if total is None:
        return dict(info, formings=1)
    out = {k: total[k] + info[k] for k in ("n_sparse", "n_dense", "hits", "pairs_evaluated", "pairs")}
    out["capacity"] = max(total["capacity"], info["capacity"])
    out["formings"] = total["formings"] + 1
    return out


def event_rows(dst_dev, src_dev, axes, method, clamp=None, capacity=None, info=None):
    """event_curves with every row clamped at `clamp`: (curves, the first float of every row), the same layout.  clamp=None is
    event_curves itself.  Otherwise, with f = clamp_value(clamp, method): one FFT-path SearchBatch over the chunk's requests, one
    threshold run at float(f) keeping `capacity` hits per request, and one sushi_hip_rows_from_hits call that writes f and the hits
    into a fresh buffer -- no whole row is formed.  The flags are then read (one host synchronisation, as SearchBatch.occurrences
    accepts): every request with more hits than `capacity` is formed densely, by match_curves into a buffer of its own and
    sushi_hip_rows_clamp from there into its place (that buffer is as large as those requests' rows).  The result is bit for bit
    clamp_rows_host(event_curves' rows, clamp, method).  capacity (None: default_capacity -- min(n_shift, max(1024, n_shift // 16)),
    and at most HIT_BYTES = 256 MiB of records per run): an int >= 0; 0 sends every request with a hit the dense way.  info: a dict
    that receives n_sparse / n_dense (requests formed from their hits / densely), hits (all requests' counts), capacity, pairs_evaluated
    / pairs (block pairs the threshold run evaluated exactly, of how many).  SushiError if a hit list is not what a threshold run
    leaves (a bug, never a property of the input).
    What it costs is the threshold run: where its pair bound excludes most block pairs at f the forming takes a fraction of
    event_curves' time, where it excludes none (a clamp near chance level) it takes a little more, and a request that overflows pays
    for both routes (DESIGN.md 3.20 has the figures)."""
    f, capacity = checked_clamp(clamp, capacity, method)
    if f is None:
        return event_curves(dst_dev, src_dev, axes, method)
    import torch
    from .curves import match_curves
    from .device import SearchBatch
    from .rows import BAD_HITS, OVERFLOW, rows_clamp_device, rows_from_hits_device, rows_table
    offs, lens = [o for a in axes for o in a.offs], [m for a in axes for m in a.lens]
    starts, n_pos = [b + a.k_lo for a in axes for b in a.bases], [a.n_shift for a in axes for _ in a.bases]
    n = len(offs)
    if capacity is None:
        capacity = default_capacity(n, max(n_pos))
    capacity = min(capacity, max(n_pos))
    batch = SearchBatch(dst_dev, src_dev, offs, lens, starts, n_pos, path="fft", method=method)
    hits, counts = batch.run_threshold(float(f), capacity)
    bounds = np.zeros(n + 1, np.int64)
    np.cumsum(np.asarray(n_pos, np.int64), out=bounds[1:])
    with torch.cuda.device(dst_dev.device):
        curves = torch.empty(int(bounds[-1]), dtype=torch.float32, device=dst_dev.device)
    flags = rows_from_hits_device(hits, counts, rows_table(bounds[:-1], n_pos), f, curves).cpu().numpy()
    if (flags & BAD_HITS).any():
        raise SushiError("event_rows: the threshold run left a hit list that is not in ascending order inside its row (request %d)"
                         % int(np.flatnonzero(flags & BAD_HITS)[0]))
    dense = np.flatnonzero(flags & OVERFLOW)
    if dense.size:
        whole, at = match_curves(dst_dev, src_dev, [offs[k] for k in dense], [lens[k] for k in dense], [starts[k] for k in dense],
                                 [n_pos[k] for k in dense], method=method)
        rows_clamp_device(whole, rows_table(bounds[dense], [n_pos[k] for k in dense], in_off=at[:-1]), method, f, out=curves)
    if info is not None:
        d = batch.diagnostics()
        info.update(n_sparse=n - int(dense.size), n_dense=int(dense.size), hits=int(counts.cpu().numpy().sum()), capacity=capacity,
                    pairs_evaluated=int(d["pairs_transformed"]), pairs=int(batch.fft_pairs))
    return curves, bounds[:-1].tolist()
