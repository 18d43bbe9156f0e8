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

from . import _native, axis
from .axis import joint_window          # noqa: F401  (public here: the axis of a group is the joint search's notion)
from .common import Record, SushiError

MAX_BYTES = 1 << 30          # curve memory of one chunk of groups (find_joint_many)

JointHost = namedtuple("JointHost", "index score row_scores row_own_index row_own_scores joint")
JointDevice = namedtuple("JointDevice", "index score row_scores row_own_index row_own_scores joint joint_offsets")


def joint_host(rows, weights, method="sqdiff_normed"):
    """sushi_hip_joint_reduce for one group in NumPy (include/sushi_hip.h states the arithmetic): rows, a list of m >= 1 float32
    arrays of one length n_shift >= 1; weights, m finite float64 values >= 0.  acc = 0.0; acc = acc + w_i * float64(R_i) row after
    row; joint = float32(acc); the answer is the first index of joint's minimum ('sqdiff_normed') or maximum ('ccoeff_normed').
    Returns a JointHost: index, score (float32), row_scores (R_i[index]), row_own_index / row_own_scores (every row's own first
    extremum), joint (the float32 joint row)."""
    axis.method_code(method)
    rows = list(rows)
    w = axis.checked_weights(weights, len(rows), "joint")
    rows = axis.checked_score_rows(rows, "joint")
    acc = np.zeros(rows[0].shape[0], np.float64)
    for r, wi in zip(rows, w):
        p = wi * r.astype(np.float64)
        acc = acc + p
    joint = acc.astype(np.float32)
    index = axis.first_extremum(joint, method)
    own = np.array([axis.first_extremum(r, method) for r in rows], np.int32)
    return JointHost(index, joint[index], np.array([r[index] for r in rows], np.float32), own,
                     np.array([r[k] for r, k in zip(rows, own)], np.float32), joint)


def _tables(rows, groups, n_curve):
    """The two tables of a joint call as arrays (rows: a JOINT_ROW_DTYPE array or (curve_off, weight) pairs; groups: a
    JOINT_GROUP_DTYPE array or (first_row, n_rows, n_shift) triples), after the checks of sushi_hip_joint_reduce."""
    rt = axis.row_table(rows)
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
    axis.check_rows_inside(rt, n_curve, np.repeat(gt["n_shift"].astype(np.int64), m), "joint")
    axis.checked_weights(rt["weight"], rt.shape[0], "joint")
    return rt, gt


def joint_reduce_device(curves, rows, groups, method="sqdiff_normed", with_curve=False, hip_stream=None):
    """One call of sushi_hip_joint_reduce on `curves`, a contiguous 1-D float32 CUDA tensor (match_curves' output).  rows:
    (curve_off, weight) each; groups: (first_row, n_rows, n_shift) each, tiling the rows in order.  Returns a JointDevice of CUDA
    tensors: index int32[n_groups], score float32[n_groups], row_scores float32[n_rows], row_own_index int32[n_rows],
    row_own_scores float32[n_rows], joint (with_curve: the joint rows back to back, float32; else None) and joint_offsets (an int64
    ndarray of n_groups + 1 entries).  Asynchronous on hip_stream (default: the current torch stream of the tensor's device)."""
    import torch
    from .device import _launch
    code = axis.method_code(method)
    axis.check_curves(curves, "joint")
    rt, gt = _tables(rows, groups, int(curves.numel()))
    n_rows, n_groups = rt.shape[0], gt.shape[0]
    offsets = np.zeros(n_groups + 1, np.int64)
    np.cumsum(gt["n_shift"].astype(np.int64), out=offsets[1:])
    L = _native.lib()
    dev = curves.device
    idx = torch.empty(n_groups, dtype=torch.int32, device=dev)
    score = torch.empty(n_groups, dtype=torch.float32, device=dev)
    row_score = torch.empty(n_rows, dtype=torch.float32, device=dev)
    row_idx = torch.empty(n_rows, dtype=torch.int32, device=dev)
    row_best = torch.empty(n_rows, dtype=torch.float32, device=dev)
    joint = torch.empty(int(offsets[-1]), dtype=torch.float32, device=dev) if with_curve else None
    _launch("sushi_hip_joint_reduce", dev, L.sushi_hip_joint_bytes(n_groups, n_rows),
            lambda mem, mem_bytes, st: L.sushi_hip_joint_reduce(
                curves.data_ptr(), int(curves.numel()), rt.ctypes.data, n_rows, gt.ctypes.data, n_groups, code, mem, mem_bytes,
                idx.data_ptr(), score.data_ptr(), row_score.data_ptr(), row_idx.data_ptr(), row_best.data_ptr(),
                None if joint is None else joint.data_ptr(), st),
            (curves, idx, score, row_score, row_idx, row_best, joint), hip_stream)
    return JointDevice(idx, score, row_score, row_idx, row_best, joint, offsets)


class JointMatch(Record):
    """What a joint search found for one group.
    delta            the group's shift in seconds, k / sample_rate: event i is found at window_centers[i] + delta;
    score            the joint score there (float32);  index: its index on the joint axis (k = k_lo + index);
    k_lo, n_shift    the joint axis: displacements k_lo .. k_lo + n_shift - 1 samples (joint_window);
    event_scores     every event's own score at the joint shift (float32 array);
    event_own_delta  where every event's lone search over the same range lands (seconds, list), event_own_scores its score;
    curve            the float32 joint row (with_curve=True), or None;
    clamp, rows_info None, or with clamp= the float32 value f the rows were clamped at (as a float) and what forming the group's chunk
                     of rows took (axis.event_rows' info).  score, curve and the own extrema are then those of the clamped rows: an
                     event_own_scores entry equal to f with its event_own_delta at index 0 (k_lo) means nothing in that event's window
                     passed.  event_scores stay the true scores at the joint shift, formed one position each."""

    def __repr__(self):
        return "JointMatch(delta=%r, score=%r, events=%d)" % (self.delta, float(self.score), len(self.event_scores))


# one group of find_joint_many: its first row among all groups' events, its events on their axis, their weights
_Group = namedtuple("_Group", "first axis weights")


def find_joint_many(stream, groups, window_sizes, weights="equal", method="sqdiff_normed", with_curve=False, max_bytes=MAX_BYTES,
                    clamp=None, capacity=None):
    """WavStream.find_joint_many (its docstring)."""
    axis.method_code(method)
    f, capacity = axis.checked_clamp(clamp, capacity, method)
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
    rate = stream.sample_rate
    plans, at = [], 0
    for (pats, centres), size, wts in zip(groups, window_sizes, weights):
        m = len(pats)
        ax = axis.event_axis(stream, offs[at:at + m], axis.pattern_lengths(lens[at:at + m]), centres, size)
        plans.append(_Group(at, ax, axis.event_weights(wts, ax.lens, per_event=False)))
        at += m
    nbytes = [4 * len(g.weights) * g.axis.n_shift for g in plans]
    out, first = [], 0
    while first < len(plans):
        last, need = first, 0
        while last < len(plans) and (last == first or need + nbytes[last] <= max_bytes):
            need += nbytes[last]
            last += 1
        if need > max_bytes:
            raise SushiError("find_joint_many: one group of %d events x %d shifts needs %d bytes of curves, max_bytes is %d"
                             % (len(plans[first].weights), plans[first].axis.n_shift, need, max_bytes))
        chunk = plans[first:last]
        info = None if f is None else {}
        curves, row_off = axis.event_rows(dst_dev, src_dev, [g.axis for g in chunk], method, clamp=f, capacity=capacity, info=info)
        res = joint_reduce_device(curves, zip(row_off, [w for g in chunk for w in g.weights]),
                                  [(g.first - chunk[0].first, len(g.weights), g.axis.n_shift) for g in chunk],
                                  method=method, with_curve=with_curve)
        idx, score, row_score, row_idx, row_best = (t.cpu().numpy() for t in res[:5])
        joint = res.joint.cpu().numpy() if with_curve else None
        if f is not None:
            # every event's true score at its group's shift: the rows hold f where nothing passes, so one position each is formed
            from .curves import match_curves
            at = [b + g.axis.k_lo + int(idx[i]) for i, g in enumerate(chunk) for b in g.axis.bases]
            row_score = match_curves(dst_dev, src_dev, [o for g in chunk for o in g.axis.offs], [m for g in chunk for m in g.axis.lens],
                                     at, [1] * len(at), method=method)[0].cpu().numpy()
        for g, grp in enumerate(chunk):
            r0, m, k_lo = grp.first - chunk[0].first, len(grp.weights), grp.axis.k_lo
            out.append(JointMatch(
                delta=(k_lo + int(idx[g])) / float(rate), score=score[g], index=int(idx[g]), k_lo=k_lo, n_shift=grp.axis.n_shift,
                event_scores=row_score[r0:r0 + m].copy(),
                event_own_delta=[(k_lo + int(k)) / float(rate) for k in row_idx[r0:r0 + m]],
                event_own_scores=row_best[r0:r0 + m].copy(), clamp=None if f is None else float(f),
                rows_info=None if info is None else axis.merge_rows_info(None, info),
                curve=None if joint is None else joint[int(res.joint_offsets[g]):int(res.joint_offsets[g + 1])].copy()))
        first = last
    return out
