"""Rates of the wide ordered tracking pass (sushi_hip_track_forward_ordered_wide + sushi_hip_track_backtrack_ordered,
sushi_hip_track_order_margins_wide).  GPU.

Device time (HIP events), median of --reps runs after a warm-up, on rows of random float32 values in [0.25, 0.75), equal weights,
SQDIFF_NORMED, step_cost 0, back 256 and penalty 0.5 in every row, at

  200 events x 240,001 shifts   (a film's worth of lines at Sushi's default +-10 s window)
   16 events x 2,880,001 shifts (+-120 s)

per shape, timed by turns in the same process:

  ordered_1024        sushi_hip_track_forward_ordered + backtrack with every reach 1024: the yardstick (2048 candidates per shift);
  wide_R              sushi_hip_track_forward_ordered_wide + backtrack with every reach R, for R = 1025, 4096 and 32767;
  margins_1024        sushi_hip_track_forward_ordered_keep + backtrack + sushi_hip_track_order_margins at reach 1024;
  margins_wide_R      the same through the wide entry points at R = 1025, 4096 and 32767;

and the workspace bytes of each.  One JSON line per shape.
Usage: python tools/track_order_wide_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("lines_10s", 200, 240001), ("wide_120s", 16, 2880001)]
WIDE = (1025, 4096, 32767)
PENALTY, BACK, GUARD = 0.5, 256, 120


def _timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def case(name, E, n_shift, reps):
    import torch
    from sushi_amd import _native, track
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    stride = n_shift + 1                                               # rows start an odd number of floats apart
    curves = torch.rand(E * stride + 8, dtype=torch.float32, device=dev, generator=gen) * 0.5 + 0.25
    rows = [(1 + e * stride, 1.0) for e in range(E)]
    state = track.TrackState(E, n_shift, dev, ordered=True)
    kept = track.TrackState(E, n_shift, dev, ordered=True, margins=True)

    def forward(fn, reach):
        def run():
            fn(curves, rows, [reach] * E, PENALTY, 0.0, BACK, state)
            return track.track_ordered_backtrack_device(state)
        return run

    def margins(fwd, back, reach):
        def run():
            fwd(curves, rows, [reach] * E, PENALTY, 0.0, BACK, kept)
            shifts = track.track_ordered_backtrack_device(kept)
            back(curves, rows, [reach] * E, [GUARD] * E, PENALTY, 0.0, BACK, kept, shifts)
        return run

    runs = {"ordered_1024": forward(track.track_ordered_device, 1024)}
    for r in WIDE:
        runs["wide_%d" % r] = forward(track.track_ordered_wide_device, r)
    runs["margins_1024"] = margins(track.track_ordered_keep_device, track.track_ordered_margins_device, 1024)
    for r in WIDE:
        runs["margins_wide_%d" % r] = margins(track.track_ordered_wide_keep_device, track.track_ordered_wide_margins_device, r)
    for run in runs.values():                                           # warm-up of each at this shape
        run()
    torch.cuda.synchronize()
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, run in runs.items():
            ms[k].append(_timed(run, torch))
    L = _native.lib()
    out = {"case": name, "events": E, "n_shift": n_shift, "reps": reps, "penalty": PENALTY, "back": BACK, "step_cost": 0.0}
    for k, v in ms.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_min"] = round(float(np.min(v)), 4)
    for r in WIDE:
        out["wide_%d_over_ordered_1024" % r] = round(out["wide_%d_ms" % r] / out["ordered_1024_ms"], 5)
        out["margins_wide_%d_over_margins_1024" % r] = round(out["margins_wide_%d_ms" % r] / out["margins_1024_ms"], 5)
    out.update({"ordered_workspace_bytes": int(L.sushi_hip_track_order_bytes(E, n_shift)),
                "wide_workspace_bytes": int(L.sushi_hip_track_order_wide_bytes(E, n_shift)),
                "margins_workspace_bytes": int(L.sushi_hip_track_order_margins_bytes(E, n_shift)),
                "margins_wide_workspace_bytes": int(L.sushi_hip_track_order_margins_wide_bytes(E, n_shift))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_order_wide_rate: needs a GPU (a rate is not measured on the CPU)")
    for shape in SHAPES:
        print(json.dumps(case(*shape, reps=a.reps)), flush=True)


if __name__ == "__main__":
    main()
