"""Where the shared shift changes: events segmented by a Viterbi pass.

A joint search (sushi_amd.joint) gives the one shift a group of events shares, but the caller has to name the groups -- and in a
programme whose second half is another cut, nobody knows them.  Here every event's exact score row (``sushi_hip_match_curves``) is
put on one shift axis, and a shift is chosen per event that minimises the sum of the events' weighted scores plus a fixed price
``penalty`` for every change of shift between consecutive events.  With one price per change this is a pass of O(events x shifts);
the groups and their borders are what the backtrack finds (include/sushi_hip.h "segmentation").

* ``path_host`` -- the arithmetic in NumPy float64, bit for bit what the kernels give; the CPU path of the pass.
* ``PathState`` / ``path_device`` / ``path_backtrack_device`` -- a sequence's device arrays, one call of
  ``sushi_hip_path_forward`` on a chunk of its rows, and the backtrack.
* ``find_segments`` -- what ``WavStream.find_segments`` runs: per chunk of events one ``match_curves`` call and one forward call,
  then one backtrack.
"""
from collections import namedtuple

import numpy as np

from . import _native, axis
from .common import Record, SushiError
from .joint import MAX_BYTES

MAX_STATE_BYTES = 2 << 30     # stay bits and D of one sequence (find_segments)

PathHost = namedtuple("PathHost", "shifts cost row_min row_arg row_own_index row_own_scores")


def _checked(weights, n, penalty, method):
    axis.method_code(method)
    w = axis.checked_weights(weights, n, "path")
    try:
        lam = float(penalty)
    except (TypeError, ValueError):
        raise SushiError("path: penalty must be a number")
    if not np.isfinite(lam) or lam < 0:
        raise SushiError("path: penalty must be finite and >= 0")
    return w, lam


def path_host(rows, weights, penalty, method="sqdiff_normed"):
    """sushi_hip_path_forward + sushi_hip_path_backtrack for one sequence in NumPy (include/sushi_hip.h states the arithmetic):
    rows, a list of E >= 1 float32 arrays of one length n_shift >= 1 in event order; weights, E finite float64 values >= 0;
    penalty, a finite number >= 0.  u_e = w_e * float64(R_e) (negated first for 'ccoeff_normed'); D_0 = u_0; m_e, a_e = the minimum
    of D_e and its first index; jump_e = m_{e-1} + penalty; stay_e = D_{e-1} <= jump_e; D_e = u_e + where(stay_e, D_{e-1}, jump_e);
    s_{E-1} = a_{E-1}, s_{e-1} = s_e if stay_e[s_e] else a_{e-1}.  Returns a PathHost: shifts (int32 index per event), cost
    (float64: m_{E-1}), row_min (float64) / row_arg (int32) per row, row_own_index / row_own_scores (every row's own first
    extremum)."""
    rows = list(rows)
    w, lam = _checked(weights, len(rows), penalty, method)
    rows = axis.checked_score_rows(rows, "path")
    E = len(rows)
    row_min = np.empty(E, np.float64)
    row_arg = np.empty(E, np.int32)
    stay = [None] * E
    D = None
    for e, (r, we) in enumerate(zip(rows, w)):
        c = r.astype(np.float64)
        if method == "ccoeff_normed":
            c = -c
        u = we * c
        if e == 0:
            D = u
        else:
            jump = row_min[e - 1] + lam
            stay[e] = D <= jump
            D = u + np.where(stay[e], D, jump)
        row_arg[e] = int(np.argmin(D))          # the first index of the minimum; 0.0 and -0.0 compare equal
        row_min[e] = D[row_arg[e]]
    shifts = np.empty(E, np.int32)
    s = int(row_arg[E - 1])
    shifts[E - 1] = s
    for e in range(E - 1, 0, -1):
        if not stay[e][s]:
            s = int(row_arg[e - 1])
        shifts[e - 1] = s
    own = np.array([axis.first_extremum(r, method) for r in rows], np.int32)
    return PathHost(shifts, float(row_min[E - 1]), row_min, row_arg, own, np.array([r[k] for r, k in zip(rows, own)], np.float32))


def runs(values):
    """Maximal runs of equal consecutive values: [(first, count, value)]."""
    out = []
    for i, v in enumerate(values):
        if out and out[-1][2] == v:
            out[-1][1] += 1
        else:
            out.append([i, 1, v])
    return [tuple(r) for r in out]


class PathState(object):
    """The device arrays of one sequence of n_total rows over n_shift shifts: D (float64[n_shift]), stay (int64[n_total * words]),
    row_min (float64[n_total]), row_arg / row_own_index (int32[n_total]), row_own_scores (float32[n_total]).  path_device fills
    them chunk by chunk; path_backtrack_device reads them."""

    def __init__(self, n_total, n_shift, device):
        import torch
        n_total, n_shift = int(n_total), int(n_shift)
        if n_total < 1 or n_shift < 1 or n_shift > 2 ** 31 - 1:
            raise SushiError("path: a sequence has >= 1 rows and 1 .. 2^31 - 1 shifts")
        self.n_total, self.n_shift, self.device = n_total, n_shift, device
        self.words = (n_shift + 63) // 64
        with torch.cuda.device(device):
            self.D = torch.empty(n_shift, dtype=torch.float64, device=device)
            self.stay = torch.empty(n_total * self.words, dtype=torch.int64, device=device)
            self.row_min = torch.empty(n_total, dtype=torch.float64, device=device)
            self.row_arg = torch.empty(n_total, dtype=torch.int32, device=device)
            self.row_own_index = torch.empty(n_total, dtype=torch.int32, device=device)
            self.row_own_scores = torch.empty(n_total, dtype=torch.float32, device=device)

    def tensors(self):
        return (self.D, self.stay, self.row_min, self.row_arg, self.row_own_index, self.row_own_scores)

    @staticmethod
    def nbytes(n_total, n_shift):
        """Bytes of stay bits and D: what grows with the sequence."""
        return int(n_total) * ((int(n_shift) + 63) // 64) * 8 + int(n_shift) * 8


def path_device(curves, rows, penalty, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """One call of sushi_hip_path_forward: rows row0 .. row0 + len(rows) - 1 of `state`'s sequence, rows[i] = (curve_off, weight)
    in `curves`, a contiguous 1-D float32 CUDA tensor (match_curves' output) on state's device.  row0 > 0 continues what the calls
    before it on the same stream left in `state`: a sequence goes through chunk by chunk, with the bits of one call.  Asynchronous
    on hip_stream (default: the current torch stream of the device)."""
    from .device import _launch
    axis.check_curves(curves, "path", device=state.D.device)
    rt = axis.row_table(rows)
    _w, lam = _checked(rt["weight"], rt.shape[0], penalty, method)
    row0 = int(row0)
    if row0 < 0 or row0 + rt.shape[0] > state.n_total:
        raise SushiError("path: rows %d .. %d are not inside a sequence of %d" % (row0, row0 + rt.shape[0] - 1, state.n_total))
    axis.check_rows_inside(rt, int(curves.numel()), state.n_shift, "path")
    L = _native.lib()
    _launch("sushi_hip_path_forward", state.D.device, L.sushi_hip_path_bytes(rt.shape[0], state.n_shift),
            lambda mem, mem_bytes, st: L.sushi_hip_path_forward(
                curves.data_ptr(), int(curves.numel()), rt.ctypes.data, rt.shape[0], state.n_shift, _native.METHODS[method], lam,
                row0, state.n_total, state.D.data_ptr(), state.stay.data_ptr(), state.row_min.data_ptr(), state.row_arg.data_ptr(),
                state.row_own_index.data_ptr(), state.row_own_scores.data_ptr(), mem, mem_bytes, st),
            (curves,) + state.tensors(), hip_stream)
    return state


def path_backtrack_device(state, hip_stream=None):
    """sushi_hip_path_backtrack over `state` once every row has gone through path_device on the same stream: the shift index of
    every row, an int32 CUDA tensor."""
    import torch
    from .device import _launch
    L = _native.lib()
    out = torch.empty(state.n_total, dtype=torch.int32, device=state.D.device)
    _launch("sushi_hip_path_backtrack", state.D.device, None,
            lambda _mem, _mem_bytes, st: L.sushi_hip_path_backtrack(state.stay.data_ptr(), state.row_arg.data_ptr(), state.n_total,
                                                                    state.n_shift, out.data_ptr(), st),
            (state.stay, state.row_arg, out), hip_stream)
    return out


class Segmentation(Record):
    """What find_segments found.
    k_lo, n_shift     the shift axis: displacements k_lo .. k_lo + n_shift - 1 samples (joint_window over all events);
    shifts            every event's displacement in samples (list of int);  deltas: the same in seconds: event i is found at
                      window_centers[i] + deltas[i];
    segments          maximal runs of equal shift: [(first_event, n_events, delta)];
    cost              the pass's total (float64): the weighted scores (negated under 'ccoeff_normed') plus penalty per change;
    event_scores      every event's own score at its chosen shift (float32 array);
    event_own_delta   where every event's lone search over the same range lands (seconds, list), event_own_scores its score;
    clamp, rows_info  None, or with clamp= the float32 value f the rows were clamped at (as a float) and what forming them took
                      (axis.event_rows' info, summed over the chunks).  The pass is then the exact minimum of the clamped problem;
                      cost and the own extrema are those of the clamped rows: an event_own_scores entry equal to f with its
                      event_own_delta at index 0 (k_lo) means nothing in that event's window passed.  event_scores stay the true
                      scores at the chosen shifts, formed one position each."""

    def __repr__(self):
        return "Segmentation(segments=%r, cost=%r)" % (self.segments, self.cost)


def find_segments(stream, patterns, window_centers, window_size, penalty, weights="equal", method="sqdiff_normed",
                  max_bytes=MAX_BYTES, max_state_bytes=MAX_STATE_BYTES, clamp=None, capacity=None):
    """WavStream.find_segments (its docstring)."""
    from .curves import match_curves
    patterns, centres = list(patterns), list(window_centers)
    if not patterns or len(patterns) != len(centres):
        raise SushiError("find_segments: equally many patterns and centres (>= 1)")
    f, capacity = axis.checked_clamp(clamp, capacity, method)
    dst_dev = stream.device_stream()
    src_dev, offs, lens, _ = stream._pattern_source(patterns, dst_dev)
    lens = axis.pattern_lengths(lens)
    E = len(patterns)
    w, lam = _checked(axis.event_weights(weights, lens, per_event=True), E, penalty, method)
    ax = axis.event_axis(stream, offs, lens, centres, window_size)
    k_lo, n_shift, rate = ax.k_lo, ax.n_shift, stream.sample_rate
    need = PathState.nbytes(E, n_shift)
    if need > max_state_bytes:
        raise SushiError("find_segments: %d events x %d shifts need %d bytes of stay bits and costs, max_state_bytes is %d"
                         % (E, n_shift, need, max_state_bytes))
    per_chunk = int(max_bytes) // (4 * n_shift)
    if per_chunk < 1:
        raise SushiError("find_segments: one event of %d shifts needs %d bytes of curves, max_bytes is %d"
                         % (n_shift, 4 * n_shift, max_bytes))
    state = PathState(E, n_shift, dst_dev.device)
    rows_info = None
    for first in range(0, E, per_chunk):
        last = min(E, first + per_chunk)
        info = {}
        curves, row_off = axis.event_rows(dst_dev, src_dev, [ax.part(first, last)], method, clamp=f, capacity=capacity, info=info)
        if f is not None:
            rows_info = axis.merge_rows_info(rows_info, info)
        path_device(curves, zip(row_off, w[first:last].tolist()), lam, state, row0=first, method=method)
    index = path_backtrack_device(state).cpu().numpy()
    shifts = [k_lo + int(k) for k in index]
    # every event's score at its chosen shift: curves are exact per position, so these are the bits of its row there
    at, _ = match_curves(dst_dev, src_dev, ax.offs, lens, [b + k for b, k in zip(ax.bases, shifts)], [1] * E, method=method)
    own = state.row_own_index.cpu().numpy()
    return Segmentation(
        k_lo=k_lo, n_shift=n_shift, shifts=shifts, deltas=[k / float(rate) for k in shifts],
        segments=[(f, n, k / float(rate)) for f, n, k in runs(shifts)], cost=float(state.row_min[E - 1].item()),
        event_scores=at.cpu().numpy(), event_own_delta=[(k_lo + int(k)) / float(rate) for k in own],
        event_own_scores=state.row_own_scores.cpu().numpy(), clamp=None if f is None else float(f), rows_info=rows_info)
