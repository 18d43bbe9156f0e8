"""A shift that wanders: events tracked by a Viterbi pass with bounded moves.

The segmentation pass (sushi_amd.segments) charges its full ``penalty`` for every change of shift, however small, and the drift
search (sushi_amd.drift) follows one straight line.  A shift that moves a little from event to event -- two captures on unlocked
clocks, an analogue source -- and may also jump at a cut falls between them.  Here, between consecutive events, the shift may
either *move* by at most ``reach_e`` samples at ``step_cost`` a sample, or *jump* anywhere at ``penalty``; the pass is exact, the
minimum over all assignments (include/sushi_hip.h "tracking").  With every reach 0 it is the segmentation pass.

* ``track_host`` -- the arithmetic in NumPy float64, bit for bit what the kernels give; the CPU path of the pass.
* ``TrackState`` / ``track_device`` / ``track_backtrack_device`` -- a sequence's device arrays, one call of
  ``sushi_hip_track_forward`` on a chunk of its rows, and the backtrack.
* ``find_track`` -- what ``WavStream.find_track`` runs: per chunk of events one ``match_curves`` call and one forward call, then
  one backtrack.
"""
import math
from collections import namedtuple

import numpy as np

from . import _native, axis
from .common import Record, SushiError
from .joint import MAX_BYTES
from .segments import _checked as _checked_path

MAX_STATE_BYTES = 2 << 30     # moves and D of one sequence (find_track)
MAX_REACH, JUMP = _native.TRACK_MAX_REACH, _native.TRACK_JUMP

TrackHost = namedtuple("TrackHost", "shifts cost row_min row_arg moves row_own_index row_own_scores")


def _checked(weights, n, penalty, step_cost, method):
    w, lam = _checked_path(weights, n, penalty, method)
    try:
        mu = float(step_cost)
    except (TypeError, ValueError):
        raise SushiError("track: step_cost must be a number")
    if not np.isfinite(mu) or mu < 0:
        raise SushiError("track: step_cost must be finite and >= 0")
    return w, lam, mu


def checked_reach(reach, n, first_row=0):
    """`reach` -- one int for every row, or a sequence of n -- as an int32 array of n values in 0 .. MAX_REACH; the value of the
    sequence's row 0 (first_row == 0: entry 0) is ignored and returned as 0.  SushiError names the row and the value otherwise."""
    try:
        r = [int(reach)] * n if np.ndim(reach) == 0 else [int(x) for x in reach]
    except (TypeError, ValueError):
        raise SushiError("track: reach is an int, or one int per row")
    if len(r) != n:
        raise SushiError("track: as many reaches as rows")
    if first_row == 0 and r:
        r[0] = 0
    for i, x in enumerate(r):
        if x < 0 or x > MAX_REACH:
            raise SushiError("track: the reach of event %d is %d, outside 0 .. %d" % (first_row + i, x, MAX_REACH))
    return np.array(r, np.int32)


def track_host(rows, weights, penalty, step_cost, reach, method="sqdiff_normed"):
    """sushi_hip_track_forward + sushi_hip_track_backtrack for one sequence in NumPy (include/sushi_hip.h states the arithmetic):
    rows, a list of E >= 1 float32 arrays of one length n_shift >= 1 in event order; weights, E finite float64 values >= 0; penalty
    and step_cost, finite numbers >= 0; reach, an int or E ints in 0 .. 1024 (row 0's is ignored).  u_e = w_e * float64(R_e) (negated
    first for 'ccoeff_normed'); D_0 = u_0; m_e, a_e = the minimum of D_e and its first index; jump_e = m_{e-1} + penalty; near_e[j]
    = the smallest of D_{e-1}[j] and D_{e-1}[j + d] + step_cost * |d| over 0 < |d| <= reach_e inside the axis, visited in the order
    0, -1, +1, -2, +2, ... with strict replacement (so the smaller |d|, then the negative d, wins a tie); D_e = u_e + where(near_e <=
    jump_e, near_e, jump_e); move_e = the winning d, or -32768 for a jump; s_{E-1} = a_{E-1}, s_{e-1} = a_{e-1} after a jump, else
    s_e + move_e[s_e].  Returns a TrackHost: shifts (int32 index per event), cost (float64: m_{E-1}), row_min (float64) / row_arg
    (int32) per row, moves (int16 [E, n_shift]; row 0's are 0), row_own_index / row_own_scores (every row's own first extremum)."""
    rows = list(rows)
    w, lam, mu = _checked(weights, len(rows), penalty, step_cost, method)
    rows = axis.checked_score_rows(rows, "track")
    E, n = len(rows), rows[0].shape[0]
    reach = checked_reach(reach, E)
    row_min = np.empty(E, np.float64)
    row_arg = np.empty(E, np.int32)
    moves = np.zeros((E, n), np.int16)
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
            near = D.copy()                          # cand(0): the value itself, nothing added
            nd = np.zeros(n, np.int16)
            for a in range(1, min(int(reach[e]), n - 1) + 1):
                price = mu * float(a)                # rounds once; the sums below round once
                lo = D[:n - a] + price               # cand(-a) of j = a .. n - 1
                take = lo < near[a:]
                near[a:][take] = lo[take]
                nd[a:][take] = -a
                hi = D[a:] + price                   # cand(+a) of j = 0 .. n - 1 - a
                take = hi < near[:n - a]
                near[:n - a][take] = hi[take]
                nd[:n - a][take] = a
            take_near = near <= jump
            D = u + np.where(take_near, near, jump)
            moves[e] = np.where(take_near, nd, np.int16(JUMP))
        row_arg[e] = int(np.argmin(D))              # the first index of the minimum; 0.0 and -0.0 compare equal
        row_min[e] = D[row_arg[e]]
    shifts = backtrack_host(moves, row_arg)
    own = np.array([axis.first_extremum(r, method) for r in rows], np.int32)
    return TrackHost(shifts, float(row_min[E - 1]), row_min, row_arg, moves, own,
                     np.array([r[k] for r, k in zip(rows, own)], np.float32))


def backtrack_host(moves, row_arg):
    """s_{E-1} = a_{E-1}; s_{e-1} = a_{e-1} where move_e[s_e] is a jump, else s_e + move_e[s_e] (clamped into the axis)."""
    E, n = moves.shape
    shifts = np.empty(E, np.int32)
    s = min(max(int(row_arg[E - 1]), 0), n - 1)
    shifts[E - 1] = s
    for e in range(E - 1, 0, -1):
        m = int(moves[e, s])
        s = int(row_arg[e - 1]) if m == JUMP else s + m
        s = min(max(s, 0), n - 1)
        shifts[e - 1] = s
    return shifts


class TrackState(object):
    """The device arrays of one sequence of n_total rows over n_shift shifts: D (float64[2 * n_shift]: two halves, used by turns),
    moves (int16[n_total * n_shift]), row_min (float64[n_total]), row_arg / row_own_index (int32[n_total]), row_own_scores
    (float32[n_total]).  track_device fills them chunk by chunk; track_backtrack_device reads them."""

    def __init__(self, n_total, n_shift, device):
        import torch
        n_total, n_shift = int(n_total), int(n_shift)
        if n_total < 1 or n_shift < 1 or n_shift > 2 ** 31 - 1:
            raise SushiError("track: a sequence has >= 1 rows and 1 .. 2^31 - 1 shifts")
        self.n_total, self.n_shift, self.device = n_total, n_shift, device
        with torch.cuda.device(device):
            self.D = torch.empty(2 * n_shift, dtype=torch.float64, device=device)
            self.moves = torch.empty(n_total * n_shift, dtype=torch.int16, device=device)
            self.row_min = torch.empty(n_total, dtype=torch.float64, device=device)
            self.row_arg = torch.empty(n_total, dtype=torch.int32, device=device)
            self.row_own_index = torch.empty(n_total, dtype=torch.int32, device=device)
            self.row_own_scores = torch.empty(n_total, dtype=torch.float32, device=device)

    def tensors(self):
        return (self.D, self.moves, self.row_min, self.row_arg, self.row_own_index, self.row_own_scores)

    def last_D(self):
        """D of the sequence's last row: the half it was written to."""
        half = (self.n_total - 1) & 1
        return self.D[half * self.n_shift:(half + 1) * self.n_shift]

    @staticmethod
    def nbytes(n_total, n_shift):
        """Bytes of moves and D: what grows with the sequence."""
        return int(n_total) * int(n_shift) * 2 + 2 * int(n_shift) * 8


def track_device(curves, rows, reach, penalty, step_cost, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """One call of sushi_hip_track_forward: rows row0 .. row0 + len(rows) - 1 of `state`'s sequence, rows[i] = (curve_off, weight)
    in `curves`, a contiguous 1-D float32 CUDA tensor (match_curves' output) on state's device, reach an int or one int per row
    of the call.  row0 > 0 continues what the calls before it on the same stream left in `state`: a sequence goes through chunk by
    chunk, with the bits of one call.  Asynchronous on hip_stream (default: the current torch stream of the device)."""
    from .device import _launch
    axis.check_curves(curves, "track", device=state.D.device)
    rt = axis.row_table(rows)
    _w, lam, mu = _checked(rt["weight"], rt.shape[0], penalty, step_cost, method)
    row0 = int(row0)
    if row0 < 0 or row0 + rt.shape[0] > state.n_total:
        raise SushiError("track: rows %d .. %d are not inside a sequence of %d" % (row0, row0 + rt.shape[0] - 1, state.n_total))
    rc = np.ascontiguousarray(checked_reach(reach, rt.shape[0], first_row=row0))
    axis.check_rows_inside(rt, int(curves.numel()), state.n_shift, "track")
    L = _native.lib()
    _launch("sushi_hip_track_forward", state.D.device, L.sushi_hip_track_bytes(rt.shape[0], state.n_shift),
            lambda mem, mem_bytes, st: L.sushi_hip_track_forward(
                curves.data_ptr(), int(curves.numel()), rt.ctypes.data, rc.ctypes.data, rt.shape[0], state.n_shift,
                _native.METHODS[method], lam, mu, row0, state.n_total, state.D.data_ptr(), state.moves.data_ptr(),
                state.row_min.data_ptr(), state.row_arg.data_ptr(), state.row_own_index.data_ptr(), state.row_own_scores.data_ptr(),
                mem, mem_bytes, st),
            (curves,) + state.tensors(), hip_stream)
    return state


def track_backtrack_device(state, hip_stream=None):
    """sushi_hip_track_backtrack over `state` once every row has gone through track_device on the same stream: the shift index of
    every row, an int32 CUDA tensor."""
    import torch
    from .device import _launch
    L = _native.lib()
    out = torch.empty(state.n_total, dtype=torch.int32, device=state.D.device)
    _launch("sushi_hip_track_backtrack", state.D.device, None,
            lambda _mem, _mem_bytes, st: L.sushi_hip_track_backtrack(state.moves.data_ptr(), state.row_arg.data_ptr(), state.n_total,
                                                                     state.n_shift, out.data_ptr(), st),
            (state.moves, state.row_arg, out), hip_stream)
    return out


def rate_reach(bases, max_rate, slack=1):
    """reach_e = ceil(max_rate * |base_e - base_{e-1}|) + slack for e >= 1, 0 for event 0: how far a shift that drifts by at most
    max_rate (a ratio: 1e-4 is 100 ppm) can have moved between two events, and `slack` samples for their own rounding."""
    try:
        rate, slack = float(max_rate), int(slack)
    except (TypeError, ValueError):
        raise SushiError("find_track: max_rate is a number, slack an int")
    if not np.isfinite(rate) or rate < 0 or slack < 0:
        raise SushiError("find_track: max_rate must be finite and >= 0, slack >= 0")
    return [0] + [int(math.ceil(rate * abs(int(b) - int(a)))) + slack for a, b in zip(bases[:-1], bases[1:])]


def jump_runs(n, jumps):
    """Maximal runs of events without a jump inside: [(first, count)] for n events of which `jumps` are entered by a jump."""
    starts = [0] + [e for e in sorted(jumps) if e > 0]
    return [(f, (starts[i + 1] if i + 1 < len(starts) else n) - f) for i, f in enumerate(starts)]


class Track(Record):
    """What find_track found.
    k_lo, n_shift     the shift axis: displacements k_lo .. k_lo + n_shift - 1 samples (joint_window over all events);
    shifts            every event's displacement in samples (list of int);  deltas: the same in seconds: event i is found at
                      window_centers[i] + deltas[i];
    reach             every event's reach in samples (event 0's is 0);
    moves             shifts[e] - shifts[e - 1] for every event (0 for event 0; after a jump: how far it went);
    jumps             the events entered by a jump (list of event numbers);
    segments          maximal runs of events without a jump: [(first_event, n_events, first_delta, last_delta)];
    cost              the pass's total (float64): the weighted scores (negated under 'ccoeff_normed') plus step_cost per sample
                      moved plus penalty per jump;
    event_scores      every event's own score at its chosen shift (float32 array);
    event_own_delta   where every event's lone search over the same range lands (seconds, list), event_own_scores its score."""

    def __repr__(self):
        return "Track(segments=%r, cost=%r)" % (self.segments, self.cost)


def find_track(stream, patterns, window_centers, window_size, penalty, max_rate=None, reach=None, step_cost=0.0, slack=1,
               weights="equal", method="sqdiff_normed", max_bytes=MAX_BYTES, max_state_bytes=MAX_STATE_BYTES):
    """WavStream.find_track (its docstring)."""
    from .curves import match_curves
    patterns, centres = list(patterns), list(window_centers)
    if not patterns or len(patterns) != len(centres):
        raise SushiError("find_track: equally many patterns and centres (>= 1)")
    if (max_rate is None) == (reach is None):
        raise SushiError("find_track: exactly one of max_rate and reach")
    dst_dev = stream.device_stream()
    src_dev, offs, lens, _ = stream._pattern_source(patterns, dst_dev)
    lens = axis.pattern_lengths(lens)
    E = len(patterns)
    w, lam, mu = _checked(axis.event_weights(weights, lens, per_event=True), E, penalty, step_cost, method)
    ax = axis.event_axis(stream, offs, lens, centres, window_size)
    k_lo, n_shift, rate = ax.k_lo, ax.n_shift, stream.sample_rate
    reach = checked_reach(rate_reach(ax.bases, max_rate, slack) if reach is None else reach, E)
    need = TrackState.nbytes(E, n_shift)
    if need > max_state_bytes:
        raise SushiError("find_track: %d events x %d shifts need %d bytes of moves and costs, max_state_bytes is %d"
                         % (E, n_shift, need, max_state_bytes))
    per_chunk = int(max_bytes) // (4 * n_shift)
    if per_chunk < 1:
        raise SushiError("find_track: one event of %d shifts needs %d bytes of curves, max_bytes is %d"
                         % (n_shift, 4 * n_shift, max_bytes))
    state = TrackState(E, n_shift, dst_dev.device)
    for first in range(0, E, per_chunk):
        last = min(E, first + per_chunk)
        curves, row_off = axis.event_curves(dst_dev, src_dev, [ax.part(first, last)], method)
        track_device(curves, zip(row_off, w[first:last].tolist()), reach[first:last], lam, mu, state, row0=first, method=method)
    index_dev = track_backtrack_device(state)
    index = index_dev.cpu().numpy()
    # the move word every event was entered by: row e's, at its chosen shift (E reads of the device array, gathered there)
    words = state.moves[index_dev.long() + n_shift * _arange_like(index_dev)].cpu().numpy()
    shifts = [k_lo + int(k) for k in index]
    jumps = [e for e in range(1, E) if int(words[e]) == JUMP]
    # every event's score at its chosen shift: curves are exact per position, so these are the bits of its row there
    at, _ = match_curves(dst_dev, src_dev, ax.offs, lens, [b + k for b, k in zip(ax.bases, shifts)], [1] * E, method=method)
    own = state.row_own_index.cpu().numpy()
    return Track(
        k_lo=k_lo, n_shift=n_shift, shifts=shifts, deltas=[k / float(rate) for k in shifts], reach=reach.tolist(),
        moves=[0] + [b - a for a, b in zip(shifts[:-1], shifts[1:])], jumps=jumps,
        segments=[(f, n, shifts[f] / float(rate), shifts[f + n - 1] / float(rate)) for f, n in jump_runs(E, jumps)],
        cost=float(state.row_min[E - 1].item()), event_scores=at.cpu().numpy(),
        event_own_delta=[(k_lo + int(k)) / float(rate) for k in own], event_own_scores=state.row_own_scores.cpu().numpy())


def _arange_like(index_dev):
    import torch
    return torch.arange(index_dev.numel(), dtype=torch.int64, device=index_dev.device)
