"""Rates of the segmentation pass (sushi_hip_path_forward + sushi_hip_path_backtrack).  GPU.

The forward call plus the backtrack -- device time (HIP events), median of --reps runs after a warm-up -- on real uint8 curves at
two shapes:

  (a) 200 events x 240,001 shifts   (a film's worth of lines at Sushi's default +-10 s window);
  (b)  16 events x 2,880,001 shifts (+-120 s),

against two baselines on the same device rows:

  torch   the same recursion as torch expressions, per event:
          u = w * R.double(); m = D.min(); stay = D <= m + lam; D = u + torch.minimum(D, m + lam)
          -- all there was before these entry points;
  curves  the sushi_hip_match_curves call that produces those rows (uint8 streams, 3 s patterns).

The pass and the torch form are timed by turns in the same process.  Also given: the backtrack alone, and the forward call's time
per step against the 20 x n_shift bytes a step moves (4 of the row, 8 + 8 of D, a bit of stay).  One JSON line per shape.
Usage: python tools/segments_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("lines_10s", 200, 240001), ("wide_120s", 16, 2880001)]
PATTERN = 36000            # 3 s at 12 kHz
PENALTY = 0.5


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def case(name, E, n_shift, reps):
    import torch
    from sushi_amd.curves import match_curves
    from sushi_amd.device import DeviceStream
    from sushi_amd.segments import PathState, path_backtrack_device, path_device
    rng = np.random.default_rng(11)
    step = 1777                                                        # rows start an odd number of samples apart
    n_dst = n_shift + PATTERN + step * E + 4096
    dst = DeviceStream(rng.integers(0, 256, n_dst, dtype=np.uint8))
    src = DeviceStream(rng.integers(0, 256, PATTERN * 16 + 4096, dtype=np.uint8))
    t_off = [(k % 16) * PATTERN + 7 for k in range(E)]
    args = (dst, src, t_off, [PATTERN] * E, [1 + step * k for k in range(E)], [n_shift] * E)
    curves = torch.empty(E * n_shift, dtype=torch.float32, device=dst.device)
    _, bounds = match_curves(*args, out=curves)
    torch.cuda.synchronize()
    rows = [(int(bounds[k]), 1.0) for k in range(E)]
    by_row = curves.view(E, n_shift)
    state = PathState(E, n_shift, dst.device)
    stay = torch.empty((E, n_shift), dtype=torch.bool, device=dst.device)

    def forward():
        path_device(curves, rows, PENALTY, state)

    def whole():
        forward()
        return path_backtrack_device(state)

    def backtrack():
        return path_backtrack_device(state)

    def torch_form():
        D = by_row[0].double()                                         # (w = 1: the product is the conversion)
        for e in range(1, E):
            u = by_row[e].double()
            jump = D.min() + PENALTY
            torch.le(D, jump, out=stay[e])
            D = u + torch.minimum(D, jump)
        return D.min()

    shifts, ref = whole(), torch_form()                                 # warm-up of both at this shape
    torch.cuda.synchronize()
    cost = float(state.row_min[E - 1].item())
    ms = {k: [] for k in ("whole", "forward", "backtrack", "torch", "curves")}
    for _ in range(reps):
        ms["whole"].append(_timed(whole, torch)[0])
        ms["torch"].append(_timed(torch_form, torch)[0])
        ms["forward"].append(_timed(forward, torch)[0])
        ms["backtrack"].append(_timed(backtrack, torch)[0])
    for _ in range(reps):
        ms["curves"].append(_timed(lambda: match_curves(*args, out=curves), torch)[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    step_bytes = 20.0 * n_shift
    return {"case": name, "events": E, "n_shift": n_shift, "reps": reps, "penalty": PENALTY,
            "pass_ms": round(med["whole"], 4), "pass_ms_min": round(float(np.min(ms["whole"])), 4),
            "forward_ms": round(med["forward"], 4), "backtrack_ms": round(med["backtrack"], 4),
            "backtrack_us_per_event": round(1e3 * med["backtrack"] / E, 3),
            "forward_us_per_step": round(1e3 * med["forward"] / E, 3), "step_bytes": step_bytes,
            "forward_GBps": round(step_bytes * E / med["forward"] / 1e6, 1),
            "torch_ms": round(med["torch"], 4), "torch_ms_min": round(float(np.min(ms["torch"])), 4),
            "pass_over_torch": round(med["whole"] / med["torch"], 4),
            "curves_ms": round(med["curves"], 4), "pass_over_curves": round(med["whole"] / med["curves"], 5),
            "cost": cost, "cost_equals_torch": bool(cost == float(ref.item())),
            "segments": int((shifts[1:] != shifts[:-1]).sum().item()) + 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("segments_rate: needs a GPU (a rate is not measured on the CPU)")
    for shape in SHAPES:
        print(json.dumps(case(*shape, reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
