"""Score rows clamped at a threshold: the two calls of include/sushi_hip.h "rows" (DESIGN.md 3.20).

A clamped row keeps every score that passes a float32 value f and holds f everywhere else (``axis.clamp_rows_host`` states the rule).
Formed from the hits of one threshold run it costs a fill and a scatter instead of a whole exact row.

* ``rows_from_hits_host`` -- ``sushi_hip_rows_from_hits`` in NumPy, tile by tile as the kernel goes: the CPU path, and what the
  kernel is compared with, flags included.
* ``rows_from_hits_device`` / ``rows_clamp_device`` -- one call of ``sushi_hip_rows_from_hits`` / ``sushi_hip_rows_clamp``.
``axis.event_rows`` is what the searches on a shift axis call.
"""
import numpy as np

from . import _native, axis
from .common import SushiError

TILE = 4096                  # floats of a tile (sushi_hip_rows_tile; csrc/rows_core.hpp ROWS_TILE)
OVERFLOW, BAD_HITS = _native.ROWS_OVERFLOW, _native.ROWS_BAD_HITS


def rows_table(out_off, n_pos, in_off=None):
    """SushiHipRowsRow records: row k is n_pos[k] floats from out_off[k] of the output buffer on (and from in_off[k] of the input
    buffer of a clamp call)."""
    out_off = np.asarray(out_off, np.int64).reshape(-1)
    t = np.zeros(out_off.shape[0], _native.ROWS_ROW_DTYPE)
    t["out_off"], t["n_pos"] = out_off, np.asarray(n_pos, np.int64).reshape(-1)
    if in_off is not None:
        t["in_off"] = np.asarray(in_off, np.int64).reshape(-1)
    return t


def _checked_table(table, n_out, n_in=None):
    t = np.ascontiguousarray(table, _native.ROWS_ROW_DTYPE).reshape(-1)
    n_pos = t["n_pos"].astype(np.int64)
    if t.shape[0] < 1 or (n_pos < 1).any():
        raise SushiError("rows: >= 1 rows of >= 1 floats")
    if (t["out_off"] < 0).any() or (t["out_off"] > int(n_out) - n_pos).any():
        raise SushiError("rows: a row leaves the output buffer")
    if n_in is not None and ((t["in_off"] < 0).any() or (t["in_off"] > int(n_in) - n_pos).any()):
        raise SushiError("rows: a row leaves the input buffer")
    return t


def _checked_fill(f):
    f = np.float32(f)
    if not np.isfinite(f):
        raise SushiError("rows: the clamp value must be a finite float32")
    return f


def rows_from_hits_host(hits, counts, table, f, out, tile=TILE):
    """sushi_hip_rows_from_hits in NumPy (include/sushi_hip.h states it): hits, int32 [n, capacity, 2] (index, score bits) records;
    counts, int64 [n]; table, SushiHipRowsRow records; f, the float32 fill; out, a 1-D float32 array that is written in place.  Tile
    by tile of `tile` floats, as the kernel goes: the tile is filled with f, then the records that a bisection of the list finds
    for it are written where their index lies in the tile; every tile checks its share of the list.  Returns the int32 flags."""
    hits = np.asarray(hits, np.int32)
    n, capacity = hits.shape[0], hits.shape[1]
    counts = np.asarray(counts, np.int64).reshape(-1)
    t = _checked_table(table, out.shape[0])
    f = _checked_fill(f)
    if hits.ndim != 3 or hits.shape[2] != 2 or counts.shape[0] != n or t.shape[0] != n or out.dtype != np.float32 or out.ndim != 1:
        raise SushiError("rows: hits [n, capacity, 2] int32, n counts, n rows, a 1-D float32 output")
    flags = np.zeros(n, np.int32)
    for k in range(n):
        off, n_pos, count = int(t["out_off"][k]), int(t["n_pos"][k]), int(counts[k])
        row = out[off:off + n_pos]
        row[:] = f
        if count < 0:
            flags[k] = BAD_HITS
            continue
        if count > capacity:
            flags[k] = OVERFLOW
            continue
        idx = hits[k, :count, 0].astype(np.int64)
        score = np.ascontiguousarray(hits[k, :count, 1]).view(np.float32)
        ok = (idx >= 0) & (idx < n_pos)
        ok[1:] &= idx[:-1] < idx[1:]
        if not ok.all():
            flags[k] = BAD_HITS
        for t0 in range(0, n_pos, tile):
            t1 = min(t0 + tile, n_pos)
            lo, hi = _lower_bound(idx, t0), _lower_bound(idx, t1)
            for j in range(lo, max(lo, hi)):
                if t0 <= idx[j] < t1:
                    row[idx[j]] = score[j]
    return flags


def _lower_bound(idx, x):
    # rows_core.hpp rows_lower_bound: the same steps on a list that is not sorted
    lo, hi = 0, idx.shape[0]
    while lo < hi:
        mid = lo + ((hi - lo) >> 1)
        if idx[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo


def _check_buffer(t, who):
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() != 1 or not t.is_cuda or not t.is_contiguous() or t.dtype != torch.float32 or \
            t.numel() < 1:
        raise SushiError("rows: %s is a contiguous 1-D float32 CUDA tensor" % who)


def rows_from_hits_device(hits, counts, table, f, out, hip_stream=None):
    """One call of sushi_hip_rows_from_hits: hits, an int32 CUDA tensor [n, capacity, 2] and counts, an int64 CUDA tensor [n], as
    SearchBatch.run_threshold returns them; table, SushiHipRowsRow records (rows_table); f, the float32 fill; out, a contiguous 1-D
    float32 CUDA tensor on the same device, written in place where the rows lie.  Returns the flags, an int32 CUDA tensor [n]: bit 0
    (OVERFLOW) where a request has more hits than capacity -- its row is all f --, bit 1 (BAD_HITS) where a list is not what a
    threshold run leaves.  Asynchronous on hip_stream (default: the current torch stream of the device)."""
    import torch
    from .device import _launch
    _check_buffer(out, "out")
    if not (isinstance(hits, torch.Tensor) and hits.is_cuda and hits.dtype == torch.int32 and hits.is_contiguous() and hits.dim() == 3
            and hits.shape[2] == 2 and hits.device == out.device):
        raise SushiError("rows: hits is a contiguous int32 CUDA tensor [n, capacity, 2] on the output's device")
    n, capacity = int(hits.shape[0]), int(hits.shape[1])
    if not (isinstance(counts, torch.Tensor) and counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous()
            and counts.dim() == 1 and counts.numel() == n and counts.device == out.device):
        raise SushiError("rows: counts is a contiguous int64 CUDA tensor [n] on the output's device")
    t = _checked_table(table, int(out.numel()))
    if t.shape[0] != n:
        raise SushiError("rows: as many rows as requests")
    f = _checked_fill(f)
    L = _native.lib()
    dev = out.device
    with torch.cuda.device(dev):
        flags = torch.empty(n, dtype=torch.int32, device=dev)
    # (capacity 0: a valid pointer all the same -- nothing is read through it)
    hp = hits.data_ptr() if hits.numel() else counts.data_ptr()
    _launch("sushi_hip_rows_from_hits", dev, L.sushi_hip_rows_bytes(n),
            lambda mem, mem_bytes, st: L.sushi_hip_rows_from_hits(hp, counts.data_ptr(), n, capacity, t.ctypes.data, float(f),
                                                                  out.data_ptr(), int(out.numel()), flags.data_ptr(), mem, mem_bytes, st),
            (hits, counts, out, flags), hip_stream)
    return flags


def rows_clamp_device(src, table, method, f, out=None, hip_stream=None):
    """One call of sushi_hip_rows_clamp: row k of the table, n_pos floats from in_off of `src` on, goes through the rule of
    axis.clamp_rows_host to out_off of `out` -- both contiguous 1-D float32 CUDA tensors on one device.  out=None (or `src` itself)
    clamps in place: every row then has in_off == out_off.  Returns out.  Asynchronous on hip_stream."""
    from .device import _launch
    code = axis.method_code(method)
    _check_buffer(src, "src")
    if out is None:
        out = src
    _check_buffer(out, "out")
    if out.device != src.device:
        raise SushiError("rows: src and out live on different devices")
    t = _checked_table(table, int(out.numel()), int(src.numel()))
    f = _checked_fill(f)
    a, b = src.data_ptr(), out.data_ptr()
    if not (a + 4 * src.numel() <= b or b + 4 * out.numel() <= a) and (a != b or (t["in_off"] != t["out_off"]).any()):
        raise SushiError("rows: buffers that overlap are taken only in place (the same tensor, every row at the same offset)")
    L = _native.lib()
    _launch("sushi_hip_rows_clamp", out.device, L.sushi_hip_rows_bytes(t.shape[0]),
            lambda mem, mem_bytes, st: L.sushi_hip_rows_clamp(src.data_ptr(), int(src.numel()), out.data_ptr(), int(out.numel()),
                                                              t.ctypes.data, t.shape[0], code, float(f), mem, mem_bytes, st),
            (src, out), hip_stream)
    return out
