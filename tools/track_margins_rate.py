"""Rates of the margins pass (sushi_hip_track_forward_keep, sushi_hip_track_margins).  GPU.

Device time (HIP events), median of --reps runs after a warm-up, on tools/track_rate.py's rows (random float32 values in [0.25,
0.75), equal weights, SQDIFF_NORMED) and its five shapes, guard 120, timed by turns in one process:

  forward        sushi_hip_track_forward (two halves of D), as tools/track_rate.py's pass but without the backtrack;
  forward_keep   sushi_hip_track_forward_keep (every row of D kept): the same kernels, another row stride;
  margins        sushi_hip_track_margins without M_dev, one call over all rows;
  margins_M      the same with M_dev: another 8-byte write per shift;
  torch          the same backward pass as torch expressions, per event: C padded with +inf by the reach on both sides, its
                 windows of 2 reach + 1 values (unfold) plus the prices, their minimum; n = C.min(); B = minimum(near, n +
                 penalty); M = D + B; C = u + B; M's minimum and index, its minimum and index outside the guard window, M at the
                 chosen shift -- what a user of the kept rows would otherwise write (its index among equal values is whatever
                 torch.min's is: the bitwise reference is track_margins_host, in the tests).

One JSON line per shape.
Usage: python tools/track_margins_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from track_rate import PENALTY, SHAPES, STEP_COST, _timed  # noqa: E402

GUARD = 120


def case(name, E, n_shift, reach, reps):
    import torch
    from sushi_amd.track import (TrackState, track_backtrack_device, track_device, track_forward_keep_device, track_margins_device)
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    stride = n_shift + 1                                               # rows start an odd number of floats apart
    curves = torch.rand(E * stride + 8, dtype=torch.float32, device=dev, generator=gen) * 0.5 + 0.25
    rows = [(1 + e * stride, 1.0) for e in range(E)]
    plain, kept = TrackState(E, n_shift, dev), TrackState(E, n_shift, dev, keep=True)
    reaches, guards = [reach] * E, [GUARD] * E
    M = torch.empty(E * n_shift, dtype=torch.float64, device=dev)
    price = torch.arange(-reach, reach + 1, device=dev).abs().double() * STEP_COST
    pad = torch.full((reach,), float("inf"), dtype=torch.float64, device=dev)
    index = torch.arange(n_shift, device=dev)
    inf = torch.full((), float("inf"), dtype=torch.float64, device=dev)

    forward = lambda: track_device(curves, rows, reaches, PENALTY, STEP_COST, plain)
    forward_keep = lambda: track_forward_keep_device(curves, rows, reaches, PENALTY, STEP_COST, kept)
    forward_keep()
    shifts = track_backtrack_device(kept)
    margins = lambda: track_margins_device(curves, rows, reaches, guards, PENALTY, STEP_COST, kept, shifts)
    margins_M = lambda: track_margins_device(curves, rows, reaches, guards, PENALTY, STEP_COST, kept, shifts, marginals=M)
    D_all = kept.D.view(E, n_shift)
    out_t = {k: torch.empty(E, dtype=torch.float64, device=dev) for k in ("through", "best", "alt")}
    arg_t = {k: torch.empty(E, dtype=torch.int64, device=dev) for k in ("best", "alt")}

    def torch_form():
        C = None
        for e in range(E - 1, -1, -1):
            u = curves[rows[e][0]:rows[e][0] + n_shift].double()        # (w = 1: the product is the conversion)
            if e == E - 1:
                Me, C = D_all[e], u
            else:
                jump = C.min() + PENALTY
                near = (torch.cat((pad, C, pad)).unfold(0, 2 * reach + 1, 1) + price).min(dim=1)[0] if reach else C
                B = torch.minimum(near, jump)
                Me, C = D_all[e] + B, u + B
            out_t["best"][e], arg_t["best"][e] = Me.min(dim=0)
            out_t["alt"][e], arg_t["alt"][e] = torch.where((index - shifts[e]).abs() > GUARD, Me, inf).min(dim=0)
            out_t["through"][e] = Me[shifts[e].long()]
        return C.min()

    fns = {"forward": forward, "forward_keep": forward_keep, "margins": margins, "margins_M": margins_M, "torch": torch_form}
    for fn in fns.values():                                             # warm-up of all at this shape
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(_timed(fn, torch)[0])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    out = {"case": name, "events": E, "n_shift": n_shift, "reach": reach, "guard": GUARD, "reps": reps, "penalty": PENALTY,
           "step_cost": STEP_COST}
    for k in fns:
        out[k + "_ms"] = round(med[k], 4)
        out[k + "_ms_min"] = round(float(np.min(ms[k])), 4)
    margin = (kept.alt - kept.through).cpu().numpy()
    out.update({"margins_over_forward": round(med["margins"] / med["forward"], 4),
                "margins_M_over_forward": round(med["margins_M"] / med["forward"], 4),
                "forward_keep_over_forward": round(med["forward_keep"] / med["forward"], 4),
                "margins_over_torch": round(med["margins"] / med["torch"], 5),
                "margins_M_over_torch": round(med["margins_M"] / med["torch"], 5),
                "candidates_G_per_s": round((E - 1) * n_shift * (2 * reach + 1) / med["margins"] / 1e6, 1),
                "forward_costs_equal": bool(torch.equal(plain.row_min.view(torch.int64), kept.row_min.view(torch.int64))),
                "best_equals_torch": bool(torch.equal(kept.best, out_t["best"])),
                "alt_equals_torch": bool(torch.equal(kept.alt, out_t["alt"])),
                "through_equals_torch": bool(torch.equal(kept.through, out_t["through"])),
                "smallest_margin": float(margin.min()), "largest_margin": float(margin.max())})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_margins_rate: needs a GPU (a rate is not measured on the CPU)")
    for shape in SHAPES:
        print(json.dumps(case(*shape, reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
