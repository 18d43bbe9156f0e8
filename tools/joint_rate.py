"""Rates of the joint reduction (sushi_hip_joint_reduce).  GPU.

sushi_hip_joint_reduce alone -- device time per call (HIP events), median of --reps calls after a warm-up -- at two shapes:

  (a) 200 groups x 16 rows x 240,001 shifts  (a film's worth of scenes at Sushi's default +-10 s window);
  (b)   4 groups x 16 rows x 2,880,001 shifts (+-120 s),

against two baselines on the same device rows:

  curves  the sushi_hip_match_curves call that produces those rows (uint8 streams, 3 s patterns);
  torch   the same result as a torch expression, one group at a time:
          (rows.double() * w[:, None]).sum(0).float().argmin()  -- all there was before this entry point.

The reduce and the torch form are timed by turns in the same process.  The reduce reads every row once (m x n_shift x 4 bytes per
group): its rate is given in GB/s of that.  One JSON line per shape.  Usage: python tools/joint_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("scenes_10s", 200, 16, 240001), ("wide_120s", 4, 16, 2880001)]
PATTERN = 36000            # 3 s at 12 kHz


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def case(name, n_groups, m, n_shift, reps):
    import torch
    from sushi_amd.curves import match_curves
    from sushi_amd.device import DeviceStream
    from sushi_amd.joint import joint_reduce_device
    rng = np.random.default_rng(11)
    n_rows = n_groups * m
    step = 1777                                                        # rows start an odd number of samples apart
    n_dst = n_shift + PATTERN + step * n_rows + 4096
    dst = DeviceStream(rng.integers(0, 256, n_dst, dtype=np.uint8))
    src = DeviceStream(rng.integers(0, 256, PATTERN * 16 + 4096, dtype=np.uint8))
    t_off = [(k % 16) * PATTERN + 7 for k in range(n_rows)]
    args = (dst, src, t_off, [PATTERN] * n_rows, [1 + step * k for k in range(n_rows)], [n_shift] * n_rows)
    curves = torch.empty(n_rows * n_shift, dtype=torch.float32, device=dst.device)
    _, bounds = match_curves(*args, out=curves)
    torch.cuda.synchronize()
    rows = [(int(bounds[k]), 1.0 / m) for k in range(n_rows)]
    groups = [(g * m, m, n_shift) for g in range(n_groups)]
    w = torch.full((m,), 1.0 / m, dtype=torch.float64, device=dst.device)
    by_group = curves.view(n_groups, m, n_shift)

    def reduce():
        return joint_reduce_device(curves, rows, groups).index

    def torch_form():
        return torch.stack([(by_group[g].double() * w[:, None]).sum(0).float().argmin() for g in range(n_groups)])

    idx, ref = reduce(), torch_form()                                   # warm-up of both at this shape
    torch.cuda.synchronize()
    agree = int((idx.long() == ref).sum())
    ms_reduce, ms_torch, ms_curves = [], [], []
    for _ in range(reps):
        ms_reduce.append(_timed(reduce, torch)[0])
        ms_torch.append(_timed(torch_form, torch)[0])
    for _ in range(reps):
        ms_curves.append(_timed(lambda: match_curves(*args, out=curves), torch)[0])
    t_r, t_t, t_c = (float(np.median(x)) for x in (ms_reduce, ms_torch, ms_curves))
    nbytes = 4.0 * n_rows * n_shift
    return {"case": name, "groups": n_groups, "rows": m, "n_shift": n_shift, "reps": reps, "row_bytes": nbytes,
            "reduce_ms": round(t_r, 4), "reduce_ms_min": round(float(np.min(ms_reduce)), 4), "reduce_GBps": round(nbytes / t_r / 1e6, 1),
            "torch_ms": round(t_t, 4), "torch_ms_min": round(float(np.min(ms_torch)), 4), "reduce_over_torch": round(t_r / t_t, 4),
            "curves_ms": round(t_c, 4), "reduce_over_curves": round(t_r / t_c, 5),
            "index_agrees_with_torch": "%d/%d" % (agree, n_groups)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("joint_rate: needs a GPU (a rate is not measured on the CPU)")
    for shape in SHAPES:
        print(json.dumps(case(*shape, reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
