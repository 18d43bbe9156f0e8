"""Rates of the drift reduction (sushi_hip_drift_reduce).  GPU.

sushi_hip_drift_reduce alone -- device time per call (HIP events around the call: the tables' upload and the three launches), median
and minimum of --reps calls after a warm-up -- at two shapes:

  (a) 64 events x 24,001 shifts x 8,641 candidates  (100 ppm over two hours at 12 kHz, a +-1 s window);
  (b) 12 events x 12,001 shifts x   661 candidates  (the shape of tests/test_drift_gpu.py's scenario),

against the torch expression of the same result one candidate at a time, on the same device rows and timed by turns with the reduce
in the same process: a gather of rows[e, j + o[d][e]], double(), the weighted sum over the events, float(), the values outside the
candidate's range set to +inf, min with its index; then the arg-min over the candidates.

The rows are random float32 values in [0.25, 0.75) (the reduce's time does not depend on the values but for the few atomics that
lower a key); equal weights, SQDIFF_NORMED, no lines written.  The offsets are drift_offsets(positions, rate_grid(...)) for events
spread evenly over the programme.  Work: events x shifts x candidates row elements per call; its rate is given in G elements / s.
One JSON line per shape.  Usage: python tools/drift_rate.py [--reps 20] [--label TEXT] [--no-baseline]
(SUSHI_HIP_LIB selects a variant library, e.g. one built with -DSUSHI_DRIFT_DB=8: build.build_native(defines=..., lib=..., obj_tag=...).)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (name, events, shifts, max_rate, samples between the first and the last event)
SHAPES = [("two_hours_100ppm", 64, 24001, 1e-4, 2 * 43200000), ("test_scenario", 12, 12001, 1e-3, 660000)]


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def case(name, n_rows, n_shift, max_rate, span, reps, label, baseline):
    import torch
    from sushi_amd import drift
    positions = [int(round(span * e / (n_rows - 1))) for e in range(n_rows)]
    anchor = drift.drift_anchor(positions)
    rates = drift.rate_grid(max_rate, max(positions[-1] - anchor, anchor - positions[0]))
    offsets = drift.drift_offsets(positions, rates, anchor)
    n_drifts = offsets.shape[0]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    stride = n_shift + 3                                                # rows an odd number of floats apart
    curves = torch.rand(n_rows * stride, generator=gen, device="cuda", dtype=torch.float32) * 0.5 + 0.25
    rows = [(e * stride + 1, 1.0 / n_rows) for e in range(n_rows)]
    rows2d = torch.as_strided(curves, (n_rows, n_shift), (stride, 1), 1)
    w = torch.full((n_rows, 1), 1.0 / n_rows, dtype=torch.float64, device="cuda")
    o_dev = torch.from_numpy(offsets.astype(np.int64)).cuda()
    _o, lo, hi = drift.checked_offsets(offsets, n_rows, n_shift)
    lo_dev, hi_dev = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    j = torch.arange(n_shift, device="cuda")
    inf = torch.full((), float("inf"), device="cuda")

    def reduce():
        return drift.drift_reduce_device(curves, rows, n_shift, offsets).best

    def torch_form():
        scores = torch.empty(n_drifts, dtype=torch.float32, device="cuda")
        index = torch.empty(n_drifts, dtype=torch.int64, device="cuda")
        for d in range(n_drifts):
            at = (j[None, :] + o_dev[d][:, None]).clamp_(0, n_shift - 1)
            line = (rows2d.gather(1, at).double() * w).sum(0).float()
            line = torch.where((j >= lo_dev[d]) & (j < hi_dev[d]), line, inf)
            scores[d], index[d] = torch.min(line, 0)
        best = scores.argmin()
        return torch.stack([best, index[best]])

    got = reduce()                                                      # warm-up at this shape
    torch.cuda.synchronize()
    out = {"case": name, "label": label, "events": n_rows, "n_shift": n_shift, "drifts": n_drifts, "reps": reps,
           "elements": float(n_rows) * n_shift * n_drifts, "answer": got.cpu().tolist()}
    ms_reduce, ms_torch = [], []
    if baseline:
        ref = torch_form()
        torch.cuda.synchronize()
        out["answer_agrees_with_torch"] = bool((got.long() == ref).all())
    for _ in range(reps):
        ms_reduce.append(_timed(reduce, torch)[0])
        if baseline:
            ms_torch.append(_timed(torch_form, torch)[0])
    t_r = float(np.median(ms_reduce))
    out.update({"reduce_ms": round(t_r, 4), "reduce_ms_min": round(float(np.min(ms_reduce)), 4),
                "reduce_Gelem_per_s": round(out["elements"] / t_r / 1e6, 1)})
    if baseline:
        t_t = float(np.median(ms_torch))
        out.update({"torch_ms": round(t_t, 3), "torch_ms_min": round(float(np.min(ms_torch)), 3), "reduce_over_torch": round(t_r / t_t, 5)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--label", default="")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("drift_rate: needs a GPU (a rate is not measured on the CPU)")
    for shape in SHAPES:
        print(json.dumps(case(*shape, reps=a.reps, label=a.label, baseline=not a.no_baseline)), flush=True)


if __name__ == "__main__":
    main()
