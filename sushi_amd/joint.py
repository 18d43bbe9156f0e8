"""The one shift a group of events shares: a joint search.

Subtitle events of one scene share one shift, and a lone search of a short line, a repeated jingle or a line over silence may find
a better decoy somewhere in its window.  Here a whole group is scored per candidate shift: every event's exact score row
(``sushi_hip_match_curves``) is put on one shift axis, the rows are summed by weight, and the group's answer is the first extremum
of the sum (include/sushi_hip.h "joint search").

* ``joint_host`` -- the arithmetic in NumPy float64, bit for bit what the kernel gives; the CPU path of the reduction.
* ``joint_reduce_device`` -- one call of ``sushi_hip_joint_reduce`` on a buffer of curves.
* ``joint_window`` -- which displacements every event of a group can take inside the stream: pure integers.
* ``find_joint_many`` -- what ``WavStream.find_joint`` / ``find_joint_many`` run: one ``match_curves`` call and one
  ``joint_reduce_device`` call per chunk of groups.
"""
from collections import namedtuple

import numpy as np

from . import _native
from .common import SushiError

MAX_BYTES = 1 << 30          # curve memory of one chunk of groups (find_joint_many)

JointHost = namedtuple("JointHost", "index score row_scores row_own_index row_own_scores joint")
JointDevice = namedtuple("JointDevice", "index score row_scores row_own_index row_own_scores joint joint_offsets")


def _first_extremum(row, method):
    # np.argmin / np.argmax return the first index of the extremum; 0.0 and -0.0 compare equal
    return int(np.argmax(row)) if method == "ccoeff_normed" else int(np.argmin(row))


def joint_host(rows, weights, method="sqdiff_normed"):
    """sushi_hip_joint_reduce for one group in NumPy (include/sushi_hip.h states the arithmetic): rows, a list of m >= 1 float32
    arrays of one length n_shift >= 1; weights, m finite float64 values >= 0.  acc = 0.0; acc = acc + w_i * float64(R_i) row after
    row; joint = float32(acc); the answer is the first index of joint's minimum ('sqdiff_normed') or maximum ('ccoeff_normed').
    Returns a JointHost: index, score (float32), row_scores (R_i[index]), row_own_index / row_own_scores (every row's own first
    extremum), joint (the float32 joint row)."""
    if method not in _native.METHODS:
        raise SushiError("method must be one of %s" % sorted(_native.METHODS))
    rows = [np.asarray(r) for r in rows]
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if not rows or w.shape[0] != len(rows):
        raise SushiError("joint: as many weights as rows (>= 1)")
    n = rows[0].shape[0] if rows[0].ndim == 1 else -1
    if n < 1 or any(r.ndim != 1 or r.dtype != np.float32 or r.shape[0] != n for r in rows):
        raise SushiError("joint: rows are 1-D float32 arrays of one length >= 1")
    if not np.isfinite(w).all() or (w < 0).any():
        raise SushiError("joint: weights must be finite and >= 0")
    acc = np.zeros(n, np.float64)
    for r, wi in zip(rows, w):
        p = wi * r.astype(np.float64)
        acc = acc + p
    joint = acc.astype(np.float32)
    index = _first_extremum(joint, method)
    own = np.array([_first_extremum(r, method) for r in rows], np.int32)
    return JointHost(index, joint[index], np.array([r[index] for r in rows], np.float32), own,
                     np.array([r[k] for r, k in zip(rows, own)], np.float32), joint)


def _tables(rows, groups, n_curve):
    """The two tables of a joint call as arrays (rows: a JOINT_ROW_DTYPE array or (curve_off, weight) pairs; groups: a
    JOINT_GROUP_DTYPE array or (first_row, n_rows, n_shift) triples), after the checks of sushi_hip_joint_reduce."""
    if isinstance(rows, np.ndarray) and rows.dtype == _native.JOINT_ROW_DTYPE:
        rt = np.ascontiguousarray(rows).reshape(-1)
    else:
        rt = np.array([(int(o), float(w)) for o, w in rows], dtype=_native.JOINT_ROW_DTYPE).reshape(-1)
    if isinstance(groups, np.ndarray) and groups.dtype == _native.JOINT_GROUP_DTYPE:
        gt = np.ascontiguousarray(groups).reshape(-1)
    else:
        gt = np.array([(int(f), int(m), int(n), 0) for f, m, n in groups], dtype=_native.JOINT_GROUP_DTYPE).reshape(-1)
    if gt.shape[0] < 1 or rt.shape[0] < 1:
        raise SushiError("joint: no groups or no rows")
    m = gt["n_rows"].astype(np.int64)
    if (m < 1).any() or (gt["n_shift"] < 1).any():
        raise SushiError("joint: a group has >= 1 rows and >= 1 shifts")
    if (gt["first_row"] != np.concatenate(([0], np.cumsum(m)[:-1]))).any() or int(m.sum()) != rt.shape[0]:
        raise SushiError("joint: the groups must tile the rows in order")
    span = np.repeat(gt["n_shift"].astype(np.int64), m)
    if (rt["curve_off"] < 0).any() or (rt["curve_off"] > n_curve - span).any():
        raise SushiError("joint: a row leaves the curve buffer")
    if not np.isfinite(rt["weight"]).all() or (rt["weight"] < 0).any():
        raise SushiError("joint: weights must be finite and >= 0")
    return rt, gt


def joint_reduce_device(curves, rows, groups, method="sqdiff_normed", with_curve=False, hip_stream=None):
    """One call of sushi_hip_joint_reduce on `curves`, a contiguous 1-D float32 CUDA tensor (match_curves' output).  rows:
    (curve_off, weight) each; groups: (first_row, n_rows, n_shift) each, tiling the rows in order.  Returns a JointDevice of CUDA
    tensors: index int32[n_groups], score float32[n_groups], row_scores float32[n_rows], row_own_index int32[n_rows],
    row_own_scores float32[n_rows], joint (with_curve: the joint rows back to back, float32; else None) and joint_offsets (an int64
    ndarray of n_groups + 1 entries).  Asynchronous on hip_stream (default: the current torch stream of the tensor's device)."""
    import torch
    from .device import _buffer, _raw_stream
    if method not in _native.METHODS:
        raise SushiError("method must be one of %s" % sorted(_native.METHODS))
    if not isinstance(curves, torch.Tensor) or curves.dim() != 1 or not curves.is_cuda or not curves.is_contiguous() or \
            curves.dtype != torch.float32 or curves.numel() < 1:
        raise SushiError("joint: a contiguous 1-D float32 CUDA tensor of curves")
    rt, gt = _tables(rows, groups, int(curves.numel()))
    n_rows, n_groups = rt.shape[0], gt.shape[0]
    offsets = np.zeros(n_groups + 1, np.int64)
    np.cumsum(gt["n_shift"].astype(np.int64), out=offsets[1:])
    L = _native.lib()
    dev = curves.device
    with torch.cuda.device(dev):
        idx = torch.empty(n_groups, dtype=torch.int32, device=dev)
        score = torch.empty(n_groups, dtype=torch.float32, device=dev)
        row_score = torch.empty(n_rows, dtype=torch.float32, device=dev)
        row_idx = torch.empty(n_rows, dtype=torch.int32, device=dev)
        row_best = torch.empty(n_rows, dtype=torch.float32, device=dev)
        joint = torch.empty(int(offsets[-1]), dtype=torch.float32, device=dev) if with_curve else None
        mem = _buffer(max(256, L.sushi_hip_joint_bytes(n_groups, n_rows)), dev)
        st = _raw_stream(dev) if hip_stream is None else hip_stream
        rc = L.sushi_hip_joint_reduce(curves.data_ptr(), int(curves.numel()), rt.ctypes.data, n_rows, gt.ctypes.data, n_groups,
                                      _native.METHODS[method], mem.data_ptr(), mem.numel(), idx.data_ptr(), score.data_ptr(),
                                      row_score.data_ptr(), row_idx.data_ptr(), row_best.data_ptr(),
                                      None if joint is None else joint.data_ptr(), st)
        _native.check(rc, "sushi_hip_joint_reduce")
        if hip_stream is not None:
            ext = torch.cuda.ExternalStream(hip_stream, device=dev)
            for t in (mem, idx, score, row_score, row_idx, row_best) + (() if joint is None else (joint,)):
                t.record_stream(ext)
    return JointDevice(idx, score, row_score, row_idx, row_best, joint, offsets)


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


class JointMatch(object):
    """What a joint search found for one group.
    delta            the group's shift in seconds, k / sample_rate: event i is found at window_centers[i] + delta;
    score            the joint score there (float32);  index: its index on the joint axis (k = k_lo + index);
    k_lo, n_shift    the joint axis: displacements k_lo .. k_lo + n_shift - 1 samples (joint_window);
    event_scores     every event's own score at the joint shift (float32 array);
    event_own_delta  where every event's lone search over the same range lands (seconds, list), event_own_scores its score;
    curve            the float32 joint row (with_curve=True), or None."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return "JointMatch(delta=%r, score=%r, events=%d)" % (self.delta, float(self.score), len(self.event_scores))


def _weights(weights, lens):
    m = len(lens)
    if isinstance(weights, str):
        if weights == "equal":
            return [1.0 / m] * m
        if weights == "length":
            total = float(sum(lens))
            return [float(n) / total for n in lens]
        raise SushiError("weights: 'equal', 'length' or a sequence of numbers")
    try:
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise SushiError("weights: 'equal', 'length' or a sequence of numbers")
    if len(w) != m:
        raise SushiError("weights: one per event of the group")
    return w


def find_joint_many(stream, groups, window_sizes, weights="equal", method="sqdiff_normed", with_curve=False, max_bytes=MAX_BYTES):
    """WavStream.find_joint_many (its docstring)."""
    from .curves import match_curves
    if method not in _native.METHODS:
        raise SushiError("method must be one of %s" % sorted(_native.METHODS))
    groups = [(list(p), list(c)) for p, c in groups]
    window_sizes = list(window_sizes)
    if not groups or len(window_sizes) != len(groups) or any(not p or len(p) != len(c) for p, c in groups):
        raise SushiError("find_joint_many: groups of equally many patterns and centres (>= 1), one window size per group")
    if isinstance(weights, str):
        weights = [weights] * len(groups)
    elif len(weights) != len(groups):
        raise SushiError("weights: 'equal', 'length', or one entry per group (each one of those or a sequence of numbers)")
    dst_dev = stream.device_stream()
    src_dev, offs, lens, _ = stream._pattern_source([p for pats, _c in groups for p in pats], dst_dev)
    total, rate = int(stream.data.shape[1]), stream.sample_rate
    plans, at = [], 0
    for (pats, centres), size, wts in zip(groups, window_sizes, weights):
        m = len(pats)
        g_lens = [int(v) for v in lens[at:at + m]]
        if min(g_lens) < 1:
            raise SushiError("empty pattern")
        bases = [stream._get_sample_for_time(c) for c in centres]
        k_lo, n_shift = joint_window(bases, g_lens, total, int(rate * size))
        plans.append((at, m, g_lens, bases, k_lo, n_shift, _weights(wts, g_lens)))
        at += m
    out, first = [], 0
    while first < len(plans):
        last, need = first, 0
        while last < len(plans) and (last == first or need + 4 * plans[last][1] * plans[last][5] <= max_bytes):
            need += 4 * plans[last][1] * plans[last][5]
            last += 1
        if need > max_bytes:
            raise SushiError("find_joint_many: one group of %d events x %d shifts needs %d bytes of curves, max_bytes is %d"
                             % (plans[first][1], plans[first][5], need, max_bytes))
        chunk = plans[first:last]
        t_off = [int(offs[a + i]) for a, m, *_ in chunk for i in range(m)]
        t_len = [n for _a, _m, g_lens, *_ in chunk for n in g_lens]
        w_start = [b + k_lo for _a, _m, _l, bases, k_lo, *_ in chunk for b in bases]
        n_pos = [n_shift for _a, m, _l, _b, _k, n_shift, _w in chunk for _ in range(m)]
        curves, bounds = match_curves(dst_dev, src_dev, t_off, t_len, w_start, n_pos, method=method)
        row_table = list(zip(bounds[:-1].tolist(), [w for *_x, wts in chunk for w in wts]))
        group_table, r0 = [], 0
        for _a, m, _l, _b, _k, n_shift, _w in chunk:
            group_table.append((r0, m, n_shift))
            r0 += m
        res = joint_reduce_device(curves, row_table, group_table, method=method, with_curve=with_curve)
        idx, score, row_score, row_idx, row_best = (t.cpu().numpy() for t in res[:5])
        joint = res.joint.cpu().numpy() if with_curve else None
        for g, ((r0, m, n_shift), (_a, _m, _l, _b, k_lo, _n, _w)) in enumerate(zip(group_table, chunk)):
            out.append(JointMatch(
                delta=(k_lo + int(idx[g])) / float(rate), score=score[g], index=int(idx[g]), k_lo=k_lo, n_shift=n_shift,
                event_scores=row_score[r0:r0 + m].copy(),
                event_own_delta=[(k_lo + int(k)) / float(rate) for k in row_idx[r0:r0 + m]],
                event_own_scores=row_best[r0:r0 + m].copy(),
                curve=None if joint is None else joint[int(res.joint_offsets[g]):int(res.joint_offsets[g + 1])].copy()))
        first = last
    return out
