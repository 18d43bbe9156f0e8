"""Rates of the tracking pass (sushi_hip_track_forward + sushi_hip_track_backtrack).  GPU.

The forward call plus the backtrack -- device time (HIP events), median of --reps runs after a warm-up -- on rows of random float32
values in [0.25, 0.75), equal weights, SQDIFF_NORMED, at

  200 events x 240,001 shifts   (a film's worth of lines at Sushi's default +-10 s window) at reach 0, 16, 128 and 1024;
   16 events x 2,880,001 shifts (+-120 s) at reach 16,

against two baselines on the same device rows, timed by turns with the pass in the same process:

  torch   the same recursion as torch expressions, per event: D padded with +inf by the reach on both sides, its windows of
          2 reach + 1 values (unfold) plus the prices step_cost * |d|, their minimum and its index; m = D.min(); D = u +
          torch.minimum(near, m + penalty) -- all there was before these entry points (its tie rule among equal candidates is
          whatever torch.min's index is: the bitwise reference is track_host, in the tests; the cost does not depend on it);
  path    sushi_hip_path_forward + sushi_hip_path_backtrack on the same rows, at reach 0 only: what the second half of D and the
          int16 moves cost.

One JSON line per shape.
Usage: python tools/track_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("lines_10s", 200, 240001, 0), ("lines_10s", 200, 240001, 16), ("lines_10s", 200, 240001, 128),
          ("lines_10s", 200, 240001, 1024), ("wide_120s", 16, 2880001, 16)]
PENALTY, STEP_COST = 0.5, 2.0 ** -12


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def case(name, E, n_shift, reach, reps):
    import torch
    from sushi_amd.segments import PathState, path_backtrack_device, path_device
    from sushi_amd.track import TrackState, track_backtrack_device, track_device
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    stride = n_shift + 1                                               # rows start an odd number of floats apart
    curves = torch.rand(E * stride + 8, dtype=torch.float32, device=dev, generator=gen) * 0.5 + 0.25
    rows = [(1 + e * stride, 1.0) for e in range(E)]
    state = TrackState(E, n_shift, dev)
    reaches = [reach] * E
    price = torch.arange(-reach, reach + 1, device=dev).abs().double() * STEP_COST
    moves = torch.empty((E, n_shift), dtype=torch.int16, device=dev)
    pad = torch.full((reach,), float("inf"), dtype=torch.float64, device=dev)

    def whole():
        track_device(curves, rows, reaches, PENALTY, STEP_COST, state)
        return track_backtrack_device(state)

    def torch_form():
        D = curves[rows[0][0]:rows[0][0] + n_shift].double()           # (w = 1: the product is the conversion)
        for e in range(1, E):
            u = curves[rows[e][0]:rows[e][0] + n_shift].double()
            jump = D.min() + PENALTY
            if reach:
                near, at = (torch.cat((pad, D, pad)).unfold(0, 2 * reach + 1, 1) + price).min(dim=1)
                moves[e] = torch.where(near <= jump, at - reach, -32768)
            else:
                near = D
                moves[e] = torch.where(near <= jump, 0, -32768)
            D = u + torch.minimum(near, jump)
        return D.min()

    shifts, ref = whole(), torch_form()                                 # warm-up of both at this shape
    torch.cuda.synchronize()
    cost = float(state.row_min[E - 1].item())
    ms = {"pass": [], "torch": []}
    if reach == 0:
        path_state = PathState(E, n_shift, dev)

        def path():
            path_device(curves, rows, PENALTY, path_state)
            return path_backtrack_device(path_state)

        path()
        ms["path"] = []
    for _ in range(reps):
        ms["pass"].append(_timed(whole, torch)[0])
        ms["torch"].append(_timed(torch_form, torch)[0])
        if reach == 0:
            ms["path"].append(_timed(path, torch)[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"case": name, "events": E, "n_shift": n_shift, "reach": reach, "reps": reps, "penalty": PENALTY, "step_cost": STEP_COST,
           "pass_ms": round(med["pass"], 4), "pass_ms_min": round(float(np.min(ms["pass"])), 4),
           "candidates_G_per_s": round((E - 1) * n_shift * (2 * reach + 1) / med["pass"] / 1e6, 1),
           "torch_ms": round(med["torch"], 4), "torch_ms_min": round(float(np.min(ms["torch"])), 4),
           "pass_over_torch": round(med["pass"] / med["torch"], 5),
           "cost": cost, "cost_equals_torch": bool(cost == float(ref.item())),
           "jumps_on_the_path": int((state.moves.view(E, n_shift)[torch.arange(E, device=dev), shifts.long()] == -32768).sum().item())}
    if reach == 0:
        out.update({"path_ms": round(med["path"], 4), "path_ms_min": round(float(np.min(ms["path"])), 4),
                    "pass_over_path": round(med["pass"] / med["path"], 4),
                    "cost_equals_path": bool(cost == float(path_state.row_min[E - 1].item()))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_rate: needs a GPU (a rate is not measured on the CPU)")
    for shape in SHAPES:
        print(json.dumps(case(*shape, reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
