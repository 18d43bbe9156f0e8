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
* ``track_ordered_host`` / ``TrackState(ordered=True)`` / ``track_ordered_device`` / ``track_ordered_backtrack_device`` -- the pass
  with events kept in order (include/sushi_hip.h "ordered tracking"): a jump into event e may lower the shift by at
  most ``back_e`` samples and costs ``penalty_e``; ``order_back`` gives the backs of a list of events; ``find_track(order=...)`` and a
  ``penalty`` per event run it.
* ``track_margins_host`` / ``track_forward_keep_device`` / ``track_margins_device`` -- how firmly each event is placed: the pass's
  min-marginals (include/sushi_hip.h "margins"), in NumPy and on the device; ``find_track(margins=True)`` runs them.
* ``wide=True`` on ``track_host``, ``track_margins_host``, ``TrackState`` and ``find_track``, and ``track_wide_device`` /
  ``track_wide_keep_device`` / ``track_wide_margins_device`` -- a reach up to 32767 where moves are free (include/sushi_hip.h "wide
  tracking"): a wide row's window minimum comes from prefix and suffix minima (``_near_wide``), bit for bit the
  candidate loop's.
* ``track_ordered_margins_host`` / ``TrackState(ordered=True, margins=True)`` / ``track_ordered_keep_device`` /
  ``track_ordered_margins_device`` -- the same for the ordered pass (include/sushi_hip.h "ordered margins");
  ``find_ordered_track(margins=True)`` runs them.
* ``wide=True`` on ``track_ordered_host`` and ``track_ordered_margins_host``, and ``track_ordered_wide_device`` /
  ``track_ordered_wide_keep_device`` / ``track_ordered_wide_margins_device`` -- the two together (include/sushi_hip.h "wide ordered
  tracking"): the ordered pass and its margins with a reach up to 32767 where moves are free;
  ``find_ordered_wide_track`` runs them.
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
WIDE_MAX_REACH = _native.TRACK_WIDE_MAX_REACH      # wide=True: the widest move, allowed where step_cost is 0

TrackHost = namedtuple("TrackHost", "shifts cost row_min row_arg moves row_own_index row_own_scores")
TrackMarginsHost = namedtuple("TrackMarginsHost", TrackHost._fields + ("D", "marginals", "through", "best", "best_arg", "alt", "alt_arg",
                                                                       "c_min"))
NO_ALT = -1                   # alt_arg where no shift lies outside the guard window
BACK_ANY = _native.TRACK_BACK_ANY        # a back that leaves a jump free to come from anywhere
TrackOrderedHost = namedtuple("TrackOrderedHost", TrackHost._fields + ("prefix_arg",))
TrackOrderedMarginsHost = namedtuple("TrackOrderedMarginsHost", TrackOrderedHost._fields + TrackMarginsHost._fields[len(TrackHost._fields):])


def _checked(weights, n, penalty, step_cost, method):
    w, lam = _checked_path(weights, n, penalty, method)
    try:
        mu = float(step_cost)
    except (TypeError, ValueError):
        raise SushiError("track: step_cost must be a number")
    if not np.isfinite(mu) or mu < 0:
        raise SushiError("track: step_cost must be finite and >= 0")
    return w, lam, mu


def checked_reach(reach, n, first_row=0, wide=False):
    """`reach` -- one int for every row, or a sequence of n -- as an int32 array of n values in 0 .. MAX_REACH (wide: 0 ..
    WIDE_MAX_REACH); the value of the sequence's row 0 (first_row == 0: entry 0) is ignored and returned as 0.  SushiError names the
    row and the value otherwise."""
    most = WIDE_MAX_REACH if wide else MAX_REACH
    try:
        r = [int(reach)] * n if np.ndim(reach) == 0 else [int(x) for x in reach]
    except (TypeError, ValueError):
        raise SushiError("track: reach is an int, or one int per row")
    if len(r) != n:
        raise SushiError("track: as many reaches as rows")
    if first_row == 0 and r:
        r[0] = 0
    for i, x in enumerate(r):
        if x < 0 or x > most:
            raise SushiError("track: the reach of event %d is %d, outside 0 .. %d" % (first_row + i, x, most))
    return np.array(r, np.int32)


def checked_wide_step_cost(reach, mu, first_row=0):
    """The wide pass's one condition: a reach above MAX_REACH (`reach`: checked_reach's array) needs a step_cost of 0.  SushiError
    names the event, the reach and the step cost otherwise."""
    if mu != 0.0:
        for i, x in enumerate(reach):
            if x > MAX_REACH:
                raise SushiError("track: the reach of event %d is %d, above %d, and step_cost is %r: a wide move is a free move.  Such a "
                                 "move costs more than a jump once step_cost * reach > penalty, so clip the reach to %d or to penalty / "
                                 "step_cost" % (first_row + i, x, MAX_REACH, mu, MAX_REACH))


def checked_guard(guard, n, first_row=0):
    """`guard` -- one int for every row, or a sequence of n -- as an int32 array of n values >= 0.  SushiError names the row and the
    value otherwise."""
    try:
        g = [int(guard)] * n if np.ndim(guard) == 0 else [int(x) for x in guard]
    except (TypeError, ValueError):
        raise SushiError("track: guard is an int, or one int per row")
    if len(g) != n:
        raise SushiError("track: as many guards as rows (%d guards, %d rows)" % (len(g), n))
    for i, x in enumerate(g):
        if x < 0 or x > 2 ** 31 - 1:
            raise SushiError("track: the guard of event %d is %d, outside 0 .. 2^31 - 1" % (first_row + i, x))
    return np.array(g, np.int32)


def _near(D, reach, mu, moves=False):
    """near[j]: the smallest of D[j] itself and D[j + d] + mu * |d| over 0 < |d| <= reach inside the axis, visited in the order 0, -1,
    +1, -2, +2, ... with strict replacement; with `moves` also the winning d (int16)."""
    n = D.shape[0]
    near = D.copy()                              # cand(0): the value itself, nothing added
    nd = np.zeros(n, np.int16) if moves else None
    for a in range(1, min(int(reach), n - 1) + 1):
        price = mu * float(a)                    # rounds once; the sums below round once
        lo = D[:n - a] + price                   # cand(-a) of j = a .. n - 1
        take = lo < near[a:]
        near[a:][take] = lo[take]
        if moves:
            nd[a:][take] = -a
        hi = D[a:] + price                       # cand(+a) of j = 0 .. n - 1 - a
        take = hi < near[:n - a]
        near[:n - a][take] = hi[take]
        if moves:
            nd[:n - a][take] = a
    return near, nd


def _block_arg_minima(D, r):
    """The axis in blocks of r values: (pF, pL, sF, sL), int64 arrays of n -- the index of the minimum of D[block's first index .. i]
    (p) and of D[i .. block's last index] (s), of equal values (0.0 and -0.0 are equal) the first (F) or the last (L)."""
    n = D.shape[0]
    nb = -(-n // r)
    B = np.full(nb * r, np.inf, np.float64)
    B[:n] = D
    B = B.reshape(nb, r)
    idx = np.arange(nb * r, dtype=np.int64).reshape(nb, r)
    pos = np.arange(r, dtype=np.int64)

    def last_record(record, index):
        at = np.maximum.accumulate(np.where(record, pos, -1), axis=1)       # the scan position of the latest record
        return np.take_along_axis(index, np.maximum(at, 0), axis=1)

    run = np.minimum.accumulate(B, axis=1)
    new_f, new_l = np.ones((nb, r), bool), np.ones((nb, r), bool)
    new_f[:, 1:] = B[:, 1:] < run[:, :-1]            # upwards: an equal value is not the first ...
    new_l[:, 1:] = B[:, 1:] <= run[:, :-1]           # ... but it is the last
    pF, pL = last_record(new_f, idx), last_record(new_l, idx)
    # downwards: the columns reversed.  The padding behind the axis's end comes first there: it is no record, and the first real
    # value is one whatever it is
    Br, idx_r = B[:, ::-1], idx[:, ::-1]
    real = idx_r < n
    first_real = real.copy()
    first_real[:, 1:] &= ~real[:, :-1]
    run = np.minimum.accumulate(Br, axis=1)
    new_f, new_l = np.ones((nb, r), bool), np.ones((nb, r), bool)
    new_f[:, 1:] = Br[:, 1:] <= run[:, :-1]          # downwards: an equal value lies lower, so it is the first ...
    new_l[:, 1:] = Br[:, 1:] < run[:, :-1]           # ... and not the last
    sF = last_record((new_f & real) | first_real, idx_r)[:, ::-1]
    sL = last_record((new_l & real) | first_real, idx_r)[:, ::-1]
    return tuple(a.reshape(-1)[:n] for a in (pF, pL, sF, sL))


def _near_wide(D, reach, mu, moves=False):
    """_near for a free move (mu is +0.0 or -0.0) in O(n) whatever the reach: adding +-0.0 changes no order, so the smallest
    candidate under (value, |d|, d > 0) is the minimum of D[j - r .. j - 1] with ties to the largest index, the minimum of D[j + 1
    .. j + r] with ties to the smallest, and D[j] itself, combined under that order; the price is added once, to the winner.  A
    window of r values is a block's suffix and the next block's prefix (blocks of r values: van Herk's form), each with its first
    and its last arg-min.  Bit for bit _near's (near, nd)."""
    if mu != 0.0:
        raise SushiError("track: the wide window minimum is for a step_cost of 0")
    n = D.shape[0]
    r = min(int(reach), n - 1)
    if r < 1:
        return D.copy(), (np.zeros(n, np.int16) if moves else None)
    pF, pL, sF, sL = _block_arg_minima(D, r)
    a = np.arange(n, dtype=np.int64)                 # a window's first index; its last is b
    b = np.minimum(a + r - 1, n - 1)
    cross = (a // r) != (b // r)                     # the window ends in the next block: its prefix there belongs to it
    # (in one block the suffix from a is the window: it starts the block, or the axis's end cut it)
    first = np.where(cross & (D[pF[b]] < D[sF[a]]), pF[b], sF[a])           # arg-min of D[a .. b], ties to the first
    last = np.where(cross & (D[pL[b]] <= D[sL[a]]), pL[b], sL[a])           # ... ties to the last
    j = np.arange(n, dtype=np.int64)
    best, bd = D.copy(), np.zeros(n, np.int64)
    # the left side of j >= 1: the window from j - r, or, where the axis's start cuts it, block 0's prefix up to j - 1
    left = np.where(j[1:] >= r, last[np.maximum(j[1:] - r, 0)], pL[j[1:] - 1])
    take = D[left] < best[1:]                        # an equal value does not beat d = 0
    best[1:][take] = D[left][take]
    bd[1:][take] = (left - j[1:])[take]
    # the right side of j <= n - 2: the window from j + 1; of equal values the smaller |d|, then the negative d, wins
    right = first[j[:-1] + 1]
    dr = right - j[:-1]
    take = (D[right] < best[:-1]) | ((D[right] == best[:-1]) & (bd[:-1] != 0) & (dr < -bd[:-1]))
    best[:-1][take] = D[right][take]
    bd[:-1][take] = dr[take]
    moved = bd != 0
    near = D.copy()                                  # cand(0): the value itself, nothing added
    near[moved] = D[(j + bd)[moved]] + np.float64(mu) * np.abs(bd[moved]).astype(np.float64)
    return near, (bd.astype(np.int16) if moves else None)


def _near_of(reach):
    """The window minimum of one row: the candidate loop up to MAX_REACH, the wide form above it."""
    return _near_wide if int(reach) > MAX_REACH else _near


def _unit_cost(row, weight, method):
    """u_e = w_e * float64(R_e), R_e negated first for 'ccoeff_normed'."""
    c = row.astype(np.float64)
    if method == "ccoeff_normed":
        c = -c
    return weight * c


def _margins_tail(shifts, D, M, guard, c_min):
    """What a margins pass reads off M once it is whole, behind the forward pass's fields: (D, M, through, best, best_arg, alt,
    alt_arg, c_min) -- through M_e[s_e]; best / best_arg the minimum of M_e and its first index; alt / alt_arg the same over the
    shifts more than guard_e from s_e (inf and NO_ALT where there are none)."""
    E, n = M.shape
    through = np.array([M[e, shifts[e]] for e in range(E)], np.float64)
    best_arg = np.array([int(np.argmin(M[e])) for e in range(E)], np.int32)
    best = np.array([M[e, best_arg[e]] for e in range(E)], np.float64)
    alt, alt_arg = np.full(E, np.inf, np.float64), np.full(E, NO_ALT, np.int32)
    j = np.arange(n, dtype=np.int64)
    for e in range(E):
        outside = np.abs(j - int(shifts[e])) > int(guard[e])
        if outside.any():
            at = int(np.argmin(np.where(outside, M[e], np.inf)))       # the first index of the minimum outside the window
            alt[e], alt_arg[e] = M[e, at], at
    return D, M, through, best, best_arg, alt, alt_arg, c_min


def track_host(rows, weights, penalty, step_cost, reach, method="sqdiff_normed", _keep=None, wide=False):
    """sushi_hip_track_forward + sushi_hip_track_backtrack for one sequence in NumPy (include/sushi_hip.h states the arithmetic):
    rows, a list of E >= 1 float32 arrays of one length n_shift >= 1 in event order; weights, E finite float64 values >= 0; penalty
    and step_cost, finite numbers >= 0; reach, an int or E ints in 0 .. 1024 (row 0's is ignored).  u_e = w_e * float64(R_e) (negated
    first for 'ccoeff_normed'); D_0 = u_0; m_e, a_e = the minimum of D_e and its first index; jump_e = m_{e-1} + penalty; near_e[j]
    = the smallest of D_{e-1}[j] and D_{e-1}[j + d] + step_cost * |d| over 0 < |d| <= reach_e inside the axis, visited in the order
    0, -1, +1, -2, +2, ... with strict replacement (so the smaller |d|, then the negative d, wins a tie); D_e = u_e + where(near_e <=
    jump_e, near_e, jump_e); move_e = the winning d, or -32768 for a jump; s_{E-1} = a_{E-1}, s_{e-1} = a_{e-1} after a jump, else
    s_e + move_e[s_e].  Returns a TrackHost: shifts (int32 index per event), cost (float64: m_{E-1}), row_min (float64) / row_arg
    (int32) per row, moves (int16 [E, n_shift]; row 0's are 0), row_own_index / row_own_scores (every row's own first extremum).
    wide=True (include/sushi_hip.h "wide tracking"): a reach may be up to 32767, and one above 1024 needs a step_cost of 0; such a
    row's near_e is _near_wide's, the same candidates and the same bits in O(n_shift); every other row's is untouched."""
    rows = list(rows)
    w, lam, mu = _checked(weights, len(rows), penalty, step_cost, method)
    rows = axis.checked_score_rows(rows, "track")
    E, n = len(rows), rows[0].shape[0]
    reach = checked_reach(reach, E, wide=wide)
    if wide:
        checked_wide_step_cost(reach, mu)
    row_min = np.empty(E, np.float64)
    row_arg = np.empty(E, np.int32)
    moves = np.zeros((E, n), np.int16)
    D = None
    for e, (r, we) in enumerate(zip(rows, w)):
        u = _unit_cost(r, we, method)
        if e == 0:
            D = u
        else:
            jump = row_min[e - 1] + lam
            near, nd = _near_of(reach[e])(D, reach[e], mu, moves=True)
            take_near = near <= jump
            D = u + np.where(take_near, near, jump)
            moves[e] = np.where(take_near, nd, np.int16(JUMP))
        row_arg[e] = int(np.argmin(D))              # the first index of the minimum; 0.0 and -0.0 compare equal
        row_min[e] = D[row_arg[e]]
        if _keep is not None:
            _keep.append(D)
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


def checked_penalties(penalty, n, first_row=0):
    """`penalty` -- one number for every row, or a sequence of n -- as a float64 array of n finite values >= 0; the value of the
    sequence's row 0 (first_row == 0: entry 0) is ignored and returned as 0.  SushiError names the row and the value otherwise."""
    try:
        p = [float(penalty)] * n if np.ndim(penalty) == 0 else [float(x) for x in penalty]
    except (TypeError, ValueError):
        raise SushiError("track: penalty is a number, or one number per row")
    if len(p) != n:
        raise SushiError("track: as many penalties as rows (%d penalties, %d rows)" % (len(p), n))
    if first_row == 0 and p:
        p[0] = 0.0
    for i, x in enumerate(p):
        if not np.isfinite(x) or x < 0:
            raise SushiError("track: the penalty of event %d is %r, not finite and >= 0" % (first_row + i, x))
    return np.array(p, np.float64)


def checked_back(back, n, first_row=0):
    """`back` -- one value for every row, or a sequence of n; an int >= 0, or -1 or None for no limit -- as an int32 array of n
    values in -1 .. 2^31 - 1.  SushiError names the row and the value otherwise."""
    try:
        b = [back] * n if back is None or np.ndim(back) == 0 else list(back)
        b = [BACK_ANY if x is None else int(x) for x in b]
    except (TypeError, ValueError):
        raise SushiError("track: a back is an int or None, one for every row or one per row")
    if len(b) != n:
        raise SushiError("track: as many backs as rows (%d backs, %d rows)" % (len(b), n))
    for i, x in enumerate(b):
        if x < BACK_ANY or x > 2 ** 31 - 1:
            raise SushiError("track: the back of event %d is %d, outside -1 .. 2^31 - 1" % (first_row + i, x))
    return np.array(b, np.int32)


def order_back(bases, lens, slack=0):
    """back_e = max(base_e - base_{e-1} - len_{e-1}, 0) + slack for e >= 1, no limit (-1) for event 0: by how much the shift may drop
    in a jump into event e if the event is to lie, in the destination, behind the end of the event in front of it -- base_e the
    destination sample of event e at shift 0, len_e its pattern's length; `slack` samples for the events' own rounding.  SushiError
    if the bases decrease."""
    try:
        bases, lens, slack = [int(b) for b in bases], [int(m) for m in lens], int(slack)
    except (TypeError, ValueError):
        raise SushiError("order_back: bases, lens and slack are ints")
    if not bases or len(bases) != len(lens) or slack < 0 or min(lens) < 0:
        raise SushiError("order_back: as many lengths (>= 0) as bases (>= 1), slack >= 0")
    for e in range(1, len(bases)):
        if bases[e] < bases[e - 1]:
            raise SushiError("order_back: event %d lies at %d, before event %d at %d: the events are not in order"
                             % (e, bases[e], e - 1, bases[e - 1]))
    return [BACK_ANY] + [max(bases[e] - bases[e - 1] - lens[e - 1], 0) + slack for e in range(1, len(bases))]


def _prefix(D):
    """(P, A): P[t] = the minimum of D[0 .. t], A[t] = the first index that attains it (a record is strictly below everything in
    front of it: 0.0 and -0.0 tie); P is D[A], so a zero keeps its sign."""
    run = np.minimum.accumulate(D)
    record = np.ones(D.shape[0], bool)
    record[1:] = D[1:] < run[:-1]
    A = np.maximum.accumulate(np.where(record, np.arange(D.shape[0], dtype=np.int64), 0)).astype(np.int32)
    return D[A], A


def _reach_back(n, back):
    """t_e(j) for every j of an axis of n: min(j + back, n - 1); n - 1 where back is BACK_ANY."""
    j = np.arange(n, dtype=np.int64)
    return np.full(n, n - 1, np.int64) if back < 0 else np.minimum(j + int(back), n - 1)


def track_ordered_host(rows, weights, penalties, step_cost, reach, back, method="sqdiff_normed", _keep=None, wide=False):
    """sushi_hip_track_forward_ordered + sushi_hip_track_backtrack_ordered for one sequence in NumPy (include/sushi_hip.h "ordered
    tracking" states the arithmetic): track_host's arguments, but penalties, a number or E finite numbers >= 0 (row 0's is ignored),
    and back, an int >= 0, -1 or None (no limit), or E of them (row 0's is not used).  u_e, D_0, m_e, a_e, near_e and the moves are
    track_host's; P_{e-1}[t] = min D_{e-1}[0 .. t], A_{e-1}[t] = its first index; t_e(j) = min(j + back_e, n_shift - 1) (n_shift - 1
    without a limit); jump_e[j] = P_{e-1}[t_e(j)] + penalty_e; D_e = u_e + where(near_e <= jump_e, near_e, jump_e); s_{E-1} = a_{E-1},
    s_{e-1} = A_{e-1}[t_e(s_e)] after a jump, else s_e + move_e[s_e].  With every back without a limit (or >= n_shift - 1) and one
    penalty this is track_host bit for bit.  Returns a TrackOrderedHost: TrackHost's fields, then prefix_arg (int32 [E, n_shift]:
    row e is A_e).  wide=True (include/sushi_hip.h "wide ordered tracking"): track_host's -- a reach may be up to 32767, and one above
    1024 needs a step_cost of 0; such a row's near_e is _near_wide's, the same bits; the jump term and every other row are untouched."""
    rows = list(rows)
    E = len(rows)
    w, _lam, mu = _checked(weights, E, 0.0, step_cost, method)
    rows = axis.checked_score_rows(rows, "track")
    n = rows[0].shape[0]
    reach = checked_reach(reach, E, wide=wide)
    if wide:
        checked_wide_step_cost(reach, mu)
    lam = checked_penalties(penalties, E)
    back = checked_back(back, E)
    row_min = np.empty(E, np.float64)
    row_arg = np.empty(E, np.int32)
    moves = np.zeros((E, n), np.int16)
    prefix_arg = np.empty((E, n), np.int32)
    D = P = None
    for e, (r, we) in enumerate(zip(rows, w)):
        u = _unit_cost(r, we, method)
        if e == 0:
            D = u
        else:
            jump = P[_reach_back(n, back[e])] + lam[e]
            near, nd = (_near_of(reach[e]) if wide else _near)(D, reach[e], mu, moves=True)
            take_near = near <= jump
            D = u + np.where(take_near, near, jump)
            moves[e] = np.where(take_near, nd, np.int16(JUMP))
        P, prefix_arg[e] = _prefix(D)
        row_arg[e] = prefix_arg[e, n - 1]           # the first index of the minimum
        row_min[e] = D[row_arg[e]]
        if _keep is not None:
            _keep.append(D)
    shifts = backtrack_ordered_host(moves, prefix_arg, back, row_arg)
    own = np.array([axis.first_extremum(r, method) for r in rows], np.int32)
    return TrackOrderedHost(shifts, float(row_min[E - 1]), row_min, row_arg, moves, own,
                            np.array([r[k] for r, k in zip(rows, own)], np.float32), prefix_arg)


def backtrack_ordered_host(moves, prefix_arg, back, row_arg):
    """s_{E-1} = a_{E-1}; s_{e-1} = A_{e-1}[t_e(s_e)] where move_e[s_e] is a jump, else s_e + move_e[s_e] (clamped into the axis)."""
    E, n = moves.shape
    shifts = np.empty(E, np.int32)
    s = min(max(int(row_arg[E - 1]), 0), n - 1)
    shifts[E - 1] = s
    for e in range(E - 1, 0, -1):
        m = int(moves[e, s])
        if m == JUMP:
            b = int(back[e])
            s = int(prefix_arg[e - 1, n - 1 if b < 0 else min(s + b, n - 1)])
        else:
            s = s + m
        s = min(max(s, 0), n - 1)
        shifts[e - 1] = s
    return shifts


def track_margins_host(rows, weights, penalty, step_cost, reach, guard, method="sqdiff_normed", wide=False):
    """sushi_hip_track_forward_keep + sushi_hip_track_backtrack + sushi_hip_track_margins for one sequence in NumPy (include/sushi_hip.h
    "margins" states the arithmetic); the arguments of track_host, and guard, an int or E ints >= 0.  C_{E-1} = u_{E-1}, M_{E-1} =
    D_{E-1}; for e = E-2 .. 0: n_{e+1} = the minimum of C_{e+1}, nearB = track_host's window minimum over C_{e+1} with reach_{e+1},
    B_e = where(nearB <= n_{e+1} + penalty, nearB, n_{e+1} + penalty), M_e = D_e + B_e, C_e = u_e + B_e.  Returns a TrackMarginsHost:
    track_host's fields, then D ([E, n] float64: every row of the forward pass), marginals ([E, n] float64: M), through (M_e[s_e]),
    best / best_arg (the minimum of M_e and its first index), alt / alt_arg (the same over the shifts more than guard_e from s_e;
    inf and -1 where there are none), c_min (n_e) -- float64 and int32 arrays of E.  wide=True: track_host's (a reach up to 32767
    where step_cost is 0; the backward window minimum of such a row is _near_wide's)."""
    rows = list(rows)
    kept = []
    fwd = track_host(rows, weights, penalty, step_cost, reach, method, _keep=kept, wide=wide)
    w, lam, mu = _checked(weights, len(rows), penalty, step_cost, method)
    rows = axis.checked_score_rows(rows, "track")
    E, n = len(rows), rows[0].shape[0]
    reach = checked_reach(reach, E, wide=wide)
    guard = checked_guard(guard, E)
    D = np.stack(kept)
    M = np.empty((E, n), np.float64)
    c_min = np.empty(E, np.float64)
    C = None
    for e in range(E - 1, -1, -1):
        u = _unit_cost(rows[e], w[e], method)
        if e == E - 1:
            C, M[e] = u, D[e]
        else:
            jump = c_min[e + 1] + lam
            near, _nd = _near_of(reach[e + 1])(C, reach[e + 1], mu)
            B = np.where(near <= jump, near, jump)
            M[e] = D[e] + B
            C = u + B
        c_min[e] = C[int(np.argmin(C))]
    return TrackMarginsHost(*(tuple(fwd) + _margins_tail(fwd.shifts, D, M, guard, c_min)))


def _suffix(C):
    """S[t] = the minimum of C[t ..], the value at the first (lowest) index that attains it (walking down, a record is at or below
    everything behind it: 0.0 and -0.0 tie, and the lower index's zero is kept)."""
    rev = C[::-1]
    run = np.minimum.accumulate(rev)
    record = np.ones(rev.shape[0], bool)
    record[1:] = rev[1:] <= run[:-1]
    at = np.maximum.accumulate(np.where(record, np.arange(rev.shape[0], dtype=np.int64), 0))
    return np.ascontiguousarray(rev[at][::-1])


def _reach_from(n, back):
    """t'_e(j) for every j of an axis of n: max(j - back, 0); 0 where back is BACK_ANY."""
    j = np.arange(n, dtype=np.int64)
    return np.zeros(n, np.int64) if back < 0 else np.maximum(j - int(back), 0)


def track_ordered_margins_host(rows, weights, penalties, step_cost, reach, back, guard, method="sqdiff_normed", _trace=None,
                               wide=False):
    """sushi_hip_track_forward_ordered_keep + sushi_hip_track_backtrack_ordered + sushi_hip_track_order_margins for one sequence in
    NumPy (include/sushi_hip.h "ordered margins" states the arithmetic); the arguments of track_ordered_host, and guard, an int or E
    ints >= 0.  C_{E-1} = u_{E-1}, M_{E-1} = D_{E-1}; S_e = _suffix(C_e); for e = E-2 .. 0: jumpB[j] = S_{e+1}[max(j - back_{e+1}, 0)] +
    penalty_{e+1} (S_{e+1}[0] without a limit), nearB = track_host's window minimum over C_{e+1} with reach_{e+1}, B_e = where(nearB <=
    jumpB, nearB, jumpB), M_e = D_e + B_e, C_e = u_e + B_e.  With every back without a limit (or >= n_shift - 1) and one penalty this
    is track_margins_host bit for bit.  Returns a TrackOrderedMarginsHost: track_ordered_host's fields, then D ([E, n] float64: every
    row of the ordered forward pass), marginals ([E, n] float64: M), through (M_e[s_e]), best / best_arg, alt / alt_arg (inf and -1
    where no shift lies outside the guard window), c_min (S_e[0]) -- as track_margins_host's.  wide=True: track_ordered_host's (a
    reach up to 32767 where step_cost is 0; the backward window minimum of such a row is _near_wide's)."""
    rows = list(rows)
    kept = []
    fwd = track_ordered_host(rows, weights, penalties, step_cost, reach, back, method, _keep=kept, wide=wide)
    E = len(rows)
    w, _lam, mu = _checked(weights, E, 0.0, step_cost, method)
    rows = axis.checked_score_rows(rows, "track")
    n = rows[0].shape[0]
    reach = checked_reach(reach, E, wide=wide)
    lam = checked_penalties(penalties, E)
    back = checked_back(back, E)
    guard = checked_guard(guard, E)
    D = np.stack(kept)
    M = np.empty((E, n), np.float64)
    c_min = np.empty(E, np.float64)
    C = S = None
    for e in range(E - 1, -1, -1):
        u = _unit_cost(rows[e], w[e], method)
        if e == E - 1:
            C, M[e] = u, D[e]
        else:
            jump = S[_reach_from(n, back[e + 1])] + lam[e + 1]
            near, _nd = (_near_of(reach[e + 1]) if wide else _near)(C, reach[e + 1], mu)
            B = np.where(near <= jump, near, jump)
            M[e] = D[e] + B
            C = u + B
        S = _suffix(C)
        c_min[e] = S[0]
        if _trace is not None:
            _trace.append((e, C, S))
    return TrackOrderedMarginsHost(*(tuple(fwd) + _margins_tail(fwd.shifts, D, M, guard, c_min)))


def wide_workspace_bytes(n_shift):
    """What a wide call's workspace holds beyond a plain call's: one row's window records -- per shift two float64 values and two
    32-bit index words, each array padded to 256 bytes (sushi_hip_track_wide_bytes - sushi_hip_track_bytes, up to the padding in
    front of them)."""
    pad = lambda b: (b + 255) // 256 * 256
    return 2 * pad(8 * int(n_shift)) + 2 * pad(4 * int(n_shift))


def ordered_wide_state_bytes(n_total, n_shift, margins=False, marginals=False):
    """What find_ordered_wide_track's max_state_bytes counts: the ordered pass's state (TrackState.nbytes(ordered=True, ...)) and a
    wide call's window records (wide_workspace_bytes: 24 bytes per shift)."""
    return TrackState.nbytes(n_total, n_shift, ordered=True, margins=margins, marginals=marginals) + wide_workspace_bytes(n_shift)


class TrackState(object):
    """The device arrays of one sequence of n_total rows over n_shift shifts: D (float64[2 * n_shift]: two halves, used by turns),
    moves (int16[n_total * n_shift]), row_min (float64[n_total]), row_arg / row_own_index (int32[n_total]), row_own_scores
    (float32[n_total]).  track_device fills them chunk by chunk; track_backtrack_device reads them.
    keep=True: D is float64[n_total * n_shift], every row of the pass (track_forward_keep_device fills it), and the state also holds
    what track_margins_device needs and fills: C (float64[2 * n_shift]: two halves), c_min, through, best, alt (float64[n_total]),
    best_arg, alt_arg (int32[n_total]).
    ordered=True (not together with keep): the state of the ordered pass (track_ordered_device fills it, chunk by chunk;
    track_ordered_backtrack_device reads it) -- also P (float64[n_shift]: the prefix minimum of the last row advanced), prefix_arg
    (int32[n_total * n_shift]: row e holds A_e) and back (int32[n_total]: every advanced row's back).
    ordered=True, margins=True: the ordered pass with its rows kept (track_ordered_keep_device fills it) -- D is float64[n_total *
    n_shift] -- and what track_ordered_margins_device needs and fills: keep=True's C and per-row outputs, and S (float64[n_shift]:
    the suffix minimum of the last row walked).
    wide=True (not together with ordered): the same arrays -- the wide pass changes no state, a move word holds +-32767 -- for
    track_wide_device, track_wide_keep_device and track_wide_margins_device; what a wide call needs beyond a plain one is its
    workspace, one row's window records (wide_workspace_bytes), which the call takes for its own duration."""

    def __init__(self, n_total, n_shift, device, keep=False, ordered=False, margins=False, wide=False):
        import torch
        n_total, n_shift = int(n_total), int(n_shift)
        if n_total < 1 or n_shift < 1 or n_shift > 2 ** 31 - 1:
            raise SushiError("track: a sequence has >= 1 rows and 1 .. 2^31 - 1 shifts")
        if wide and ordered:
            raise SushiError("track: the ordered pass keeps its reach of %d (no wide form of it is built)" % MAX_REACH)
        self.wide = bool(wide)
        if keep and ordered:
            raise SushiError("track: the ordered pass keeps no rows (its margins are not built)")
        if margins and not ordered:
            raise SushiError("track: margins= belongs to a TrackState(ordered=True); the plain pass keeps its rows with keep=True")
        margins = bool(margins)
        keep = bool(keep) or margins                # D holds every row
        self.n_total, self.n_shift, self.device, self.keep, self.ordered = n_total, n_shift, device, keep, bool(ordered)
        self.margins = margins
        with torch.cuda.device(device):
            if ordered:
                self.P = torch.empty(n_shift, dtype=torch.float64, device=device)
                self.prefix_arg = torch.empty(n_total * n_shift, dtype=torch.int32, device=device)
                self.back = torch.empty(n_total, dtype=torch.int32, device=device)
            self.D = torch.empty((n_total if keep else 2) * n_shift, dtype=torch.float64, device=device)
            self.moves = torch.empty(n_total * n_shift, dtype=torch.int16, device=device)
            self.row_min = torch.empty(n_total, dtype=torch.float64, device=device)
            self.row_arg = torch.empty(n_total, dtype=torch.int32, device=device)
            self.row_own_index = torch.empty(n_total, dtype=torch.int32, device=device)
            self.row_own_scores = torch.empty(n_total, dtype=torch.float32, device=device)
            if keep:
                self.C = torch.empty(2 * n_shift, dtype=torch.float64, device=device)
                self.c_min, self.through, self.best, self.alt = (torch.empty(n_total, dtype=torch.float64, device=device)
                                                                 for _ in range(4))
                self.best_arg, self.alt_arg = (torch.empty(n_total, dtype=torch.int32, device=device) for _ in range(2))
            if margins:
                self.S = torch.empty(n_shift, dtype=torch.float64, device=device)

    def tensors(self):
        return (self.D, self.moves, self.row_min, self.row_arg, self.row_own_index, self.row_own_scores)

    def margin_tensors(self):
        return (self.C, self.c_min, self.through, self.best, self.best_arg, self.alt, self.alt_arg)

    def order_tensors(self):
        return (self.P, self.prefix_arg, self.back)

    def last_D(self):
        """D of the sequence's last row: the half (keep: the row) it was written to."""
        half = (self.n_total - 1) if self.keep else (self.n_total - 1) & 1
        return self.D[half * self.n_shift:(half + 1) * self.n_shift]

    @staticmethod
    def nbytes(n_total, n_shift, keep=False, marginals=False, ordered=False, margins=False, wide=False):
        """Bytes of moves and D: what grows with the sequence.  keep: every row of D and the two halves of C; marginals: M too;
        ordered: moves and A, 6 bytes per (event, shift), the two halves of D and P; ordered with margins: moves, A and every row of
        D, 14 bytes per (event, shift), the two halves of C, P and S, and M with marginals.  wide (the plain pass alone): a wide
        call's window records as well (wide_workspace_bytes: 24 bytes per shift)."""
        n_total, n_shift = int(n_total), int(n_shift)
        if wide:
            if ordered:
                raise SushiError("track: the ordered pass keeps its reach of %d (no wide form of it is built)" % MAX_REACH)
            return TrackState.nbytes(n_total, n_shift, keep=keep, marginals=marginals) + wide_workspace_bytes(n_shift)
        if ordered and margins:
            return n_total * n_shift * 14 + 2 * n_shift * 8 + 2 * n_shift * 8 + (n_total * n_shift * 8 if marginals else 0)
        if ordered:
            return n_total * n_shift * 6 + 2 * n_shift * 8 + n_shift * 8
        if not keep:
            return n_total * n_shift * 2 + 2 * n_shift * 8
        return n_total * n_shift * 2 + n_total * n_shift * 8 + 2 * n_shift * 8 + (n_total * n_shift * 8 if marginals else 0)


def track_device(curves, rows, reach, penalty, step_cost, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """One call of sushi_hip_track_forward: rows row0 .. row0 + len(rows) - 1 of `state`'s sequence, rows[i] = (curve_off, weight)
    in `curves`, a contiguous 1-D float32 CUDA tensor (match_curves' output) on state's device, reach an int or one int per row
    of the call.  row0 > 0 continues what the calls before it on the same stream left in `state`: a sequence goes through chunk by
    chunk, with the bits of one call.  Asynchronous on hip_stream (default: the current torch stream of the device)."""
    if getattr(state, "keep", False):
        raise SushiError("track: a state that keeps its rows goes through track_forward_keep_device")
    return _forward_device(False, False, False, curves, rows, reach, penalty, step_cost, None, state, row0, method, hip_stream)


def track_forward_keep_device(curves, rows, reach, penalty, step_cost, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """track_device through sushi_hip_track_forward_keep: `state` is a TrackState(keep=True), and row e of its D is D_e afterwards.
    Everything else -- arguments, the other outputs and their bits, chunks -- is track_device's."""
    if not getattr(state, "keep", False):
        raise SushiError("track: track_forward_keep_device needs a TrackState(keep=True)")
    return _forward_device(False, True, False, curves, rows, reach, penalty, step_cost, None, state, row0, method, hip_stream)


def track_wide_device(curves, rows, reach, penalty, step_cost, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """track_device through sushi_hip_track_forward_wide: a reach may be up to WIDE_MAX_REACH, and one above MAX_REACH needs a
    step_cost of 0 (SushiError otherwise).  Rows of a reach up to MAX_REACH go through track_device's own kernels: with no wider
    reach the outputs are track_device's bit for bit.  `state`: any TrackState that does not keep its rows."""
    if getattr(state, "keep", False):
        raise SushiError("track: a state that keeps its rows goes through track_wide_keep_device")
    return _forward_device(False, False, True, curves, rows, reach, penalty, step_cost, None, state, row0, method, hip_stream)


def track_wide_keep_device(curves, rows, reach, penalty, step_cost, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """track_forward_keep_device through sushi_hip_track_forward_wide_keep (track_wide_device's reaches)."""
    if not getattr(state, "keep", False):
        raise SushiError("track: track_wide_keep_device needs a TrackState(keep=True)")
    return _forward_device(False, True, True, curves, rows, reach, penalty, step_cost, None, state, row0, method, hip_stream)


def track_ordered_device(curves, rows, reach, penalties, step_cost, back, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """One call of sushi_hip_track_forward_ordered: track_device's arguments, but penalties (a number, or one per row of the call)
    and back (an int >= 0, -1 or None for no limit, or one per row of the call), and `state` a TrackState(ordered=True).  row0 > 0
    continues what the calls before it on the same stream left in `state` -- D, and P of the last row advanced: a sequence goes
    through chunk by chunk, with the bits of one call.  Three launches per row; measured at 64 rows x 2.88 M shifts, 12.3 x
    track_device's time at reach 0 and 2.8 x at reach 88 (profiles/track_order/).  Asynchronous on hip_stream."""
    if not getattr(state, "ordered", False):
        raise SushiError("track: track_ordered_device needs a TrackState(ordered=True)")
    if getattr(state, "margins", False):
        raise SushiError("track: a state that keeps its rows goes through track_ordered_keep_device")
    return _forward_device(True, False, False, curves, rows, reach, penalties, step_cost, back, state, row0, method, hip_stream)


def track_ordered_keep_device(curves, rows, reach, penalties, step_cost, back, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """track_ordered_device through sushi_hip_track_forward_ordered_keep: `state` is a TrackState(ordered=True, margins=True), and row
    e of its D is D_e afterwards.  Everything else -- arguments, the other outputs and their bits, chunks -- is track_ordered_device's."""
    if not (getattr(state, "ordered", False) and getattr(state, "margins", False)):
        raise SushiError("track: track_ordered_keep_device needs a TrackState(ordered=True, margins=True)")
    return _forward_device(True, True, False, curves, rows, reach, penalties, step_cost, back, state, row0, method, hip_stream)


def track_ordered_wide_device(curves, rows, reach, penalties, step_cost, back, state, row0=0, method="sqdiff_normed", hip_stream=None):
    """track_ordered_device through sushi_hip_track_forward_ordered_wide: a reach may be up to WIDE_MAX_REACH, and one above MAX_REACH
    needs a step_cost of 0 (SushiError otherwise).  Rows of a reach up to MAX_REACH go through track_ordered_device's own kernels:
    with no wider reach the outputs are track_ordered_device's bit for bit.  `state`: an ordinary TrackState(ordered=True) -- a wide
    call changes no state, and a sequence may mix the two calls; what it needs beyond it is its workspace."""
    if not getattr(state, "ordered", False):
        raise SushiError("track: track_ordered_wide_device needs a TrackState(ordered=True)")
    if getattr(state, "margins", False):
        raise SushiError("track: a state that keeps its rows goes through track_ordered_wide_keep_device")
    return _forward_device(True, False, True, curves, rows, reach, penalties, step_cost, back, state, row0, method, hip_stream)


def track_ordered_wide_keep_device(curves, rows, reach, penalties, step_cost, back, state, row0=0, method="sqdiff_normed",
                                   hip_stream=None):
    """track_ordered_keep_device through sushi_hip_track_forward_ordered_wide_keep (track_ordered_wide_device's reaches)."""
    if not (getattr(state, "ordered", False) and getattr(state, "margins", False)):
        raise SushiError("track: track_ordered_wide_keep_device needs a TrackState(ordered=True, margins=True)")
    return _forward_device(True, True, True, curves, rows, reach, penalties, step_cost, back, state, row0, method, hip_stream)


def _forward_device(ordered, keep, wide, curves, rows, reach, penalty, step_cost, back, state, row0, method, hip_stream):
    """The forward launcher: one call of sushi_hip_track_forward[_ordered][_wide][_keep].  ordered: penalty is the call's penalties
    and back its backs (plain: one penalty, no back); wide: the reach's bound, the free-move condition and the workspace are the
    wide call's."""
    from .device import _launch
    if not ordered and getattr(state, "ordered", False):
        raise SushiError("track: a TrackState(ordered=True) goes through track_ordered_device")
    axis.check_curves(curves, "track", device=state.D.device)
    rt = axis.row_table(rows)
    n_rows = rt.shape[0]
    _w, lam, mu = _checked(rt["weight"], n_rows, 0.0 if ordered else penalty, step_cost, method)
    row0 = int(row0)
    if row0 < 0 or row0 + n_rows > state.n_total:
        raise SushiError("track: rows %d .. %d are not inside a sequence of %d" % (row0, row0 + n_rows - 1, state.n_total))
    rc = np.ascontiguousarray(checked_reach(reach, n_rows, first_row=row0, wide=wide))
    if wide:
        checked_wide_step_cost(rc, mu, first_row=row0)
    tables, outputs = (rc,), state.tensors()
    if ordered:
        pc = np.ascontiguousarray(checked_penalties(penalty, n_rows, first_row=row0))
        tables += (np.ascontiguousarray(checked_back(back, n_rows, first_row=row0)),)
        outputs = outputs[:2] + state.order_tensors() + outputs[2:]        # D, moves; P, A, back; the per-row outputs
        lam = pc.ctypes.data                                               # the penalty argument: a table, not one number
    axis.check_rows_inside(rt, int(curves.numel()), state.n_shift, "track")
    L = _native.lib()
    name = "sushi_hip_track_forward%s%s%s" % ("_ordered" if ordered else "", "_wide" if wide else "", "_keep" if keep else "")
    fn = getattr(L, name)
    bytes_fn = getattr(L, "sushi_hip_track%s%s_bytes" % ("_order" if ordered else "", "_wide" if wide else ""))
    _launch(name, state.D.device, bytes_fn(n_rows, state.n_shift),
            lambda mem, mem_bytes, st: fn(
                curves.data_ptr(), int(curves.numel()), rt.ctypes.data, *[t.ctypes.data for t in tables], n_rows, state.n_shift,
                _native.METHODS[method], lam, mu, row0, state.n_total, *[t.data_ptr() for t in outputs], mem, mem_bytes, st),
            (curves,) + state.tensors() + (state.order_tensors() if ordered else ()), hip_stream)
    return state


def track_margins_device(curves, rows, reach, guard, penalty, step_cost, state, shifts, row0=0, method="sqdiff_normed", marginals=None,
                         hip_stream=None, _wide=False):
    """One call of sushi_hip_track_margins: rows row0 + len(rows) - 1 down to row0 of `state`'s sequence (a TrackState(keep=True) whose
    every row has gone through track_forward_keep_device), `shifts` the int32 CUDA tensor track_backtrack_device returned.  rows[i] =
    (curve_off, weight) and guard[i] are row row0 + i's (guard: an int, or one per row of the call); reach: an int, or one int per
    row of the call and then the reach of row row0 + len(rows) where that row exists (the step out of the call's last row).  The
    first call of a sequence ends at its last row; a later one continues downwards from what the call before it on the same stream
    left in `state`, with the bits of one call.  marginals: a float64 CUDA tensor of n_total * n_shift values that receives M, or
    None.  Fills rows row0 .. of state.c_min, through, best, best_arg, alt, alt_arg.  Asynchronous on hip_stream."""
    if not getattr(state, "keep", False):
        raise SushiError("track: track_margins_device needs a TrackState(keep=True)")
    return _margins_device(False, _wide, curves, rows, reach, guard, penalty, step_cost, None, state, shifts, row0, method, marginals,
                           hip_stream)


def track_wide_margins_device(curves, rows, reach, guard, penalty, step_cost, state, shifts, row0=0, method="sqdiff_normed",
                              marginals=None, hip_stream=None):
    """track_margins_device through sushi_hip_track_margins_wide (track_wide_device's reaches)."""
    return track_margins_device(curves, rows, reach, guard, penalty, step_cost, state, shifts, row0=row0, method=method,
                                marginals=marginals, hip_stream=hip_stream, _wide=True)


def track_ordered_margins_device(curves, rows, reach, guard, penalties, step_cost, back, state, shifts, row0=0, method="sqdiff_normed",
                                 marginals=None, hip_stream=None, _wide=False):
    """One call of sushi_hip_track_order_margins: rows row0 + len(rows) - 1 down to row0 of `state`'s sequence (a TrackState(ordered=True,
    margins=True) whose every row has gone through track_ordered_keep_device), `shifts` the int32 CUDA tensor
    track_ordered_backtrack_device returned.  track_margins_device's arguments, but reach, penalties and back are each a single value,
    or one per row of the call and then that of row row0 + len(rows) where that row exists (the step out of the call's last row); entry
    0 is not used.  The first call of a sequence ends at its last row; a later one continues downwards from what the call before it on
    the same stream left in `state` (C and S), with the bits of one call.  Fills rows row0 .. of state.c_min, through, best, best_arg,
    alt, alt_arg, and of marginals where given.  Three launches per row.  Asynchronous on hip_stream."""
    if not (getattr(state, "ordered", False) and getattr(state, "margins", False)):
        raise SushiError("track: track_ordered_margins_device needs a TrackState(ordered=True, margins=True)")
    return _margins_device(True, _wide, curves, rows, reach, guard, penalties, step_cost, back, state, shifts, row0, method, marginals,
                           hip_stream)


def track_ordered_wide_margins_device(curves, rows, reach, guard, penalties, step_cost, back, state, shifts, row0=0,
                                      method="sqdiff_normed", marginals=None, hip_stream=None):
    """track_ordered_margins_device through sushi_hip_track_order_margins_wide (track_ordered_wide_device's reaches)."""
    return track_ordered_margins_device(curves, rows, reach, guard, penalties, step_cost, back, state, shifts, row0=row0, method=method,
                                        marginals=marginals, hip_stream=hip_stream, _wide=True)


def _margins_device(ordered, wide, curves, rows, reach, guard, penalty, step_cost, back, state, shifts, row0, method, marginals,
                    hip_stream):
    """The margins launcher: one call of sushi_hip_track[_order]_margins[_wide].  What is given per row -- reach, and with `ordered`
    penalty and back -- is a single value, or one per row of the call and then that of row row0 + len(rows) where that row exists:
    entries 1 .. n_after are used, entry 0 is not."""
    from .device import _launch
    import torch
    axis.check_curves(curves, "track", device=state.D.device)
    rt = axis.row_table(rows)
    n_rows = rt.shape[0]
    _w, lam, mu = _checked(rt["weight"], n_rows, 0.0 if ordered else penalty, step_cost, method)
    row0 = int(row0)
    if row0 < 0 or row0 + n_rows > state.n_total:
        raise SushiError("track: rows %d .. %d are not inside a sequence of %d" % (row0, row0 + n_rows - 1, state.n_total))
    n_after = n_rows + (1 if row0 + n_rows < state.n_total else 0)

    def per_row(values, what, fill):
        values = [values] * n_after if values is None or np.ndim(values) == 0 else list(values)
        if len(values) != n_after:
            raise SushiError("track: %d %s for a margins call of %d rows that %s the sequence's last row (%d are needed)"
                             % (len(values), what, n_rows, "ends below" if n_after > n_rows else "ends at", n_after))
        return [fill] + values[1:]                                                              # entry 0 is not used

    rc = np.ascontiguousarray(checked_reach(per_row(reach, "reaches", 0), n_after, first_row=row0, wide=wide))
    if wide:
        checked_wide_step_cost(rc, mu, first_row=row0)
    tables, held = (rc,), (state.C,)
    if ordered:
        pc = np.ascontiguousarray(checked_penalties(per_row(penalty, "penalties", 0.0), n_after, first_row=row0))
        tables += (np.ascontiguousarray(checked_back(per_row(back, "backs", BACK_ANY), n_after, first_row=row0)),)
        held += (state.S,)
        lam = pc.ctypes.data                                               # the penalty argument: a table, not one number
    tables += (np.ascontiguousarray(checked_guard(guard, n_rows, first_row=row0)),)
    axis.check_rows_inside(rt, int(curves.numel()), state.n_shift, "track")
    if not (isinstance(shifts, torch.Tensor) and shifts.is_cuda and shifts.dtype == torch.int32 and shifts.is_contiguous()
            and shifts.numel() == state.n_total and shifts.device == state.D.device):
        raise SushiError("track: shifts is the backtrack's output, an int32 CUDA tensor of %d values" % state.n_total)
    if marginals is not None and not (isinstance(marginals, torch.Tensor) and marginals.is_cuda and marginals.dtype == torch.float64
                                      and marginals.is_contiguous() and marginals.numel() == state.n_total * state.n_shift
                                      and marginals.device == state.D.device):
        raise SushiError("track: marginals is a contiguous float64 CUDA tensor of %d x %d values" % (state.n_total, state.n_shift))
    L = _native.lib()
    name = "sushi_hip_track%s_margins%s" % ("_order" if ordered else "", "_wide" if wide else "")
    fn = getattr(L, name)
    outputs = held + state.margin_tensors()[1:]                                                  # C (, S); c_min .. alt_arg
    _launch(name, state.D.device, getattr(L, name + "_bytes")(n_rows, state.n_shift),
            lambda mem, mem_bytes, st: fn(
                curves.data_ptr(), int(curves.numel()), rt.ctypes.data, *[t.ctypes.data for t in tables], n_rows, state.n_shift,
                _native.METHODS[method], lam, mu, row0, state.n_total, state.D.data_ptr(), shifts.data_ptr(),
                *[t.data_ptr() for t in outputs], None if marginals is None else marginals.data_ptr(), mem, mem_bytes, st),
            (curves, shifts, state.D) + held[1:] + state.margin_tensors() + (() if marginals is None else (marginals,)), hip_stream)
    return state


def track_backtrack_device(state, hip_stream=None):
    """sushi_hip_track_backtrack over `state` once every row has gone through track_device on the same stream: the shift index of
    every row, an int32 CUDA tensor."""
    return _backtrack_device(False, state, hip_stream)


def track_ordered_backtrack_device(state, hip_stream=None):
    """sushi_hip_track_backtrack_ordered over `state` once every row has gone through track_ordered_device on the same stream: the
    shift index of every row, an int32 CUDA tensor."""
    if not getattr(state, "ordered", False):
        raise SushiError("track: track_ordered_backtrack_device needs a TrackState(ordered=True)")
    return _backtrack_device(True, state, hip_stream)


def _backtrack_device(ordered, state, hip_stream):
    """The backtrack launcher: one call of sushi_hip_track_backtrack[_ordered] (ordered: A and the backs are read as well)."""
    import torch
    from .device import _launch
    name = "sushi_hip_track_backtrack" + ("_ordered" if ordered else "")
    fn = getattr(_native.lib(), name)
    out = torch.empty(state.n_total, dtype=torch.int32, device=state.D.device)
    read = (state.moves,) + ((state.prefix_arg, state.back) if ordered else ()) + (state.row_arg,)
    _launch(name, state.D.device, None,
            lambda _mem, _mem_bytes, st: fn(*[t.data_ptr() for t in read], state.n_total, state.n_shift, out.data_ptr(), st),
            read + (out,), hip_stream)
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
    event_own_delta   where every event's lone search over the same range lands (seconds, list), event_own_scores its score;
    clamp, rows_info  None, or with clamp= the float32 value f the rows were clamped at (as a float) and what forming them took
                      (axis.event_rows' info, summed over every forming of a chunk, the second one for margins included).  The pass
                      -- and its margins -- is then the exact minimum of the clamped problem; cost and the own extrema are those of
                      the clamped rows: an event_own_scores entry equal to f with its event_own_delta at index 0 (k_lo) means
                      nothing in that event's window passed.  event_scores stay the true scores at the chosen shifts, formed one
                      position each.
    back, penalties   None, or through the ordered pass (order=, a penalty per event) every event's back in samples (None: no
                      limit; event 0's is None) and every event's penalty (event 0's is 0): a jump into event e lowers the shift by
                      at most back[e] and costs penalties[e].
    With margins=True (else None), how firmly every event is placed:
    guard             every event's guard in samples (list of int);
    event_through     the cost of the best whole path through every event's chosen shift (float64 array: the total, up to
                      summation order);
    event_margin      by how much the pass's total rises if the event must lie more than `guard` samples from its place (float64
                      array: the best alternative's cost minus event_through; inf where the axis holds no such shift).  It counts
                      what the neighbours pay as well -- an alternative may move a whole run of events -- and is at most 2 *
                      penalty plus the event's own weighted score difference.  A margin far below the penalty says that the run the
                      event lies in has a second explanation nearly as good; it is not a probability and not an error in samples;
    event_alt_shift   where the event goes in that best alternative (samples; None where there is none), event_alt_delta the same
                      in seconds;
    marginals         with marginals=True, the whole min-marginals: a float64 CUDA tensor [events, n_shift], entry [e, j] the cost
                      of the best path that puts event e at displacement k_lo + j."""

    def __repr__(self):
        return "Track(segments=%r, cost=%r)" % (self.segments, self.cost)


def find_track(stream, patterns, window_centers, window_size, penalty, max_rate=None, reach=None, step_cost=0.0, slack=1,
               weights="equal", method="sqdiff_normed", max_bytes=MAX_BYTES, max_state_bytes=MAX_STATE_BYTES, margins=False,
               guard=None, marginals=False, clamp=None, capacity=None, order=None, wide=False):
    """WavStream.find_track (its docstring)."""
    wide = bool(wide)
    patterns, centres, margins, marginals = _checked_search("find_track", patterns, window_centers, max_rate, reach, margins, guard,
                                                            marginals)
    # the ordered pass is taken only when it is asked for; otherwise the code path, the launches and the bits are those of before
    order = None if order is False else order
    ordered = order is not None or (penalty is not None and np.ndim(penalty) != 0)
    if ordered:
        if wide:
            raise SushiError("find_track: wide=True belongs to the plain pass; the ordered pass (order=, a penalty per event) keeps "
                             "its reach of %d" % MAX_REACH)
        if margins:
            raise SushiError("find_track: margins of the ordered pass (order=, a penalty per event) are not built: its backward "
                             "recurrence needs the mirrored suffix minimum")
    return _search("find_track", ordered, wide, stream, patterns, centres, window_size, penalty, order, max_rate, reach, step_cost, slack,
                   weights, method, max_bytes, max_state_bytes, margins, guard, marginals, clamp, capacity)


def find_ordered_track(stream, patterns, window_centers, window_size, penalty, order=None, max_rate=None, reach=None, step_cost=0.0,
                       slack=1, weights="equal", method="sqdiff_normed", max_bytes=MAX_BYTES, max_state_bytes=MAX_STATE_BYTES,
                       margins=False, guard=None, marginals=False, clamp=None, capacity=None, wide=False):
    """WavStream.find_ordered_track (its docstring)."""
    if wide:
        raise SushiError("find_ordered_track: wide=True belongs to find_track's plain pass; the ordered pass keeps its reach of %d"
                         % MAX_REACH)
    return _find_ordered("find_ordered_track", False, stream, patterns, window_centers, window_size, penalty, order, max_rate, reach,
                         step_cost, slack, weights, method, max_bytes, max_state_bytes, margins, guard, marginals, clamp, capacity)


def find_ordered_wide_track(stream, patterns, window_centers, window_size, penalty, order=None, max_rate=None, reach=None, step_cost=0.0,
                            slack=1, weights="equal", method="sqdiff_normed", max_bytes=MAX_BYTES, max_state_bytes=MAX_STATE_BYTES,
                            margins=False, guard=None, marginals=False, clamp=None, capacity=None):
    """WavStream.find_ordered_wide_track (its docstring)."""
    return _find_ordered("find_ordered_wide_track", True, stream, patterns, window_centers, window_size, penalty, order, max_rate, reach,
                         step_cost, slack, weights, method, max_bytes, max_state_bytes, margins, guard, marginals, clamp, capacity)


def _find_ordered(name, wide, stream, patterns, window_centers, window_size, penalty, order, max_rate, reach, step_cost, slack, weights,
                  method, max_bytes, max_state_bytes, margins, guard, marginals, clamp, capacity):
    patterns, centres, margins, marginals = _checked_search(name, patterns, window_centers, max_rate, reach, margins, guard, marginals)
    return _search(name, True, wide, stream, patterns, centres, window_size, penalty, None if order is False else order, max_rate, reach,
                   step_cost, slack, weights, method, max_bytes, max_state_bytes, margins, guard, marginals, clamp, capacity)


def _checked_search(name, patterns, window_centers, max_rate, reach, margins, guard, marginals):
    """What every find_* checks first about its own arguments: (patterns, centres, margins, marginals)."""
    patterns, centres = list(patterns), list(window_centers)
    if not patterns or len(patterns) != len(centres):
        raise SushiError("%s: equally many patterns and centres (>= 1)" % name)
    if (max_rate is None) == (reach is None):
        raise SushiError("%s: exactly one of max_rate and reach" % name)
    margins, marginals = bool(margins), bool(marginals)
    if not margins and (marginals or guard is not None):
        raise SushiError("%s: guard and marginals belong to margins=True" % name)
    return patterns, centres, margins, marginals


def _search(name, ordered, wide, stream, patterns, centres, window_size, penalty, order, max_rate, reach, step_cost, slack, weights,
            method, max_bytes, max_state_bytes, margins, guard, marginals, clamp, capacity):
    """The search behind find_track, find_ordered_track and find_ordered_wide_track: per chunk of events one match_curves call and
    one forward call, then one backtrack; with margins the rows of the forward pass are kept, and the chunks are walked again from
    the last one down.  ordered: penalty is a number or one per event, and order None (every back without a limit: a penalty per
    event alone), True (order_back of the events) or one back per event; the state holds the jump sources, and the record the backs
    and the penalties.  wide: the reach's bound is WIDE_MAX_REACH, the calls are the wide ones, and the state's count holds a wide
    call's window records."""
    import torch
    from .curves import match_curves
    f, capacity = axis.checked_clamp(clamp, capacity, method)
    dst_dev = stream.device_stream()
    src_dev, offs, lens, _ = stream._pattern_source(patterns, dst_dev)
    lens = axis.pattern_lengths(lens)
    E = len(patterns)
    w, lam, mu = _checked(axis.event_weights(weights, lens, per_event=True), E, 0.0 if ordered else penalty, step_cost, method)
    if ordered:
        lam = checked_penalties(penalty, E)
    ax = axis.event_axis(stream, offs, lens, centres, window_size)
    k_lo, n_shift, rate = ax.k_lo, ax.n_shift, stream.sample_rate
    reach = checked_reach(rate_reach(ax.bases, max_rate, slack) if reach is None else reach, E, wide=wide)
    if wide:
        checked_wide_step_cost(reach, mu)
    back = None
    if ordered:
        back = checked_back(None if order is None else (order_back(ax.bases, lens) if order is True else order), E)
        back[0] = BACK_ANY
    if margins:
        guard = checked_guard(int(0.01 * rate) if guard is None else guard, E)

    def state_bytes(margins=False, marginals=False):
        if not ordered:
            return TrackState.nbytes(E, n_shift, keep=margins, marginals=marginals, wide=wide)
        return (ordered_wide_state_bytes(E, n_shift, margins=margins, marginals=marginals) if wide else
                TrackState.nbytes(E, n_shift, ordered=True, margins=margins, marginals=marginals))

    need = state_bytes(margins, marginals)
    if need > max_state_bytes:
        held = "moves, jump sources" if ordered else "moves"
        records = ", a wide call's window records" if wide else ""
        if margins:
            raise SushiError("%s: %d events x %d shifts need %d bytes of %s, kept costs%s%s, max_state_bytes is %d (%d "
                             "without margins)" % (name, E, n_shift, need, held, " and marginals" if marginals else "", records,
                                                   max_state_bytes, state_bytes()))
        raise SushiError("%s: %d events x %d shifts need %d bytes of %s and costs%s, max_state_bytes is %d"
                         % (name, E, n_shift, need, held, records, max_state_bytes))
    per_chunk = int(max_bytes) // (4 * n_shift)
    if per_chunk < 1:
        raise SushiError("%s: one event of %d shifts needs %d bytes of curves, max_bytes is %d"
                         % (name, n_shift, 4 * n_shift, max_bytes))
    if ordered:
        state = TrackState(E, n_shift, dst_dev.device, ordered=True, margins=margins)
    else:
        state = TrackState(E, n_shift, dst_dev.device, keep=margins, wide=wide)
    chunks = [(first, min(E, first + per_chunk)) for first in range(0, E, per_chunk)]
    rows_info = [None]

    def form(first, last):
        info = {}
        formed = axis.event_rows(dst_dev, src_dev, [ax.part(first, last)], method, clamp=f, capacity=capacity, info=info)
        if f is not None:
            rows_info[0] = axis.merge_rows_info(rows_info[0], info)
        return formed

    def per_row(first, upto):                   # (penalty, back) of rows first .. upto - 1: the ordered pass's per-row arrays
        return (lam[first:upto], back[first:upto]) if ordered else (lam, None)

    for first, last in chunks:
        curves, row_off = form(first, last)
        price, backs = per_row(first, last)
        _forward_device(ordered, margins, wide, curves, zip(row_off, w[first:last].tolist()), reach[first:last], price, mu, backs, state,
                        first, method, None)
    index_dev = _backtrack_device(ordered, state, None)
    extra = dict(guard=None, event_through=None, event_margin=None, event_alt_shift=None, event_alt_delta=None, marginals=None)
    if margins:
        # the chunks again, from the last one down: a lone chunk's curves are still there, several chunks' are formed a second time
        M = torch.empty(E * n_shift, dtype=torch.float64, device=state.D.device) if marginals else None
        for first, last in reversed(chunks):
            if len(chunks) > 1:
                curves, row_off = form(first, last)
            upto = last + 1 if last < E else last
            price, backs = per_row(first, upto)
            _margins_device(ordered, wide, curves, zip(row_off, w[first:last].tolist()), reach[first:upto], guard[first:last], price, mu,
                            backs, state, index_dev, first, method, M, None)
        through, alt, alt_arg = state.through.cpu().numpy(), state.alt.cpu().numpy(), state.alt_arg.cpu().numpy()
        alt_shift = [None if int(k) == NO_ALT else k_lo + int(k) for k in alt_arg]
        extra = dict(guard=guard.tolist(), event_through=through,
                     event_margin=np.where(alt_arg == NO_ALT, np.inf, alt - through), event_alt_shift=alt_shift,
                     event_alt_delta=[None if k is None else k / float(rate) for k in alt_shift],
                     marginals=None if M is None else M.view(E, n_shift))
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
        segments=[(s, n, shifts[s] / float(rate), shifts[s + n - 1] / float(rate)) for s, n in jump_runs(E, jumps)],
        cost=float(state.row_min[E - 1].item()), event_scores=at.cpu().numpy(),
        event_own_delta=[(k_lo + int(k)) / float(rate) for k in own], event_own_scores=state.row_own_scores.cpu().numpy(),
        clamp=None if f is None else float(f), rows_info=rows_info[0],
        back=None if back is None else [None if int(b) == BACK_ANY else int(b) for b in back],
        penalties=lam.tolist() if ordered else None, **extra)


def _arange_like(index_dev):
    import torch
    return torch.arange(index_dev.numel(), dtype=torch.int64, device=index_dev.device)
