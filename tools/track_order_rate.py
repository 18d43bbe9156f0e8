"""What keeping tracked events in order costs (order=, a penalty per event).  GPU.

Forward pass: sushi_hip_track_forward_ordered against sushi_hip_track_forward of the same build on the same rows -- 64 rows of
2,880,001 shifts (random float32 scores), every reach 0 and every reach 88, backs of 36,000 shifts -- the two by turns in one
process, a host clock around a device synchronise, median of --reps runs after a warm-up, with the spread.  The plain pass is one
launch per row; the ordered one is three (the step, a scan of one record per work item, the prefix minimum of the row).

End to end: find_track with and without order=True, and with clamp=0.5 under 'ccoeff_normed', on 64 events of 3 s cut from a 2-h
12 kHz source that is the destination advanced by 30 s, +-120 s windows (the same n_shift), reach 16: whole calls, timed the same
way.

One JSON line per case.
Usage: python tools/track_order_rate.py [--reps 7] [--rows 64] [--shifts 2880001] [--events 64] [--hours 2] [--skip-find]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

RATE, EVENT_S, WINDOW, OFFSET_S = 12000, 3.0, 120.0, 30.0
PENALTY, REACH, BACK = 0.5, 16, 36000


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _stats(ms, name):
    ms = np.array(ms)
    return {name + "_ms": round(float(np.median(ms)), 3), name + "_ms_min": round(float(ms.min()), 3),
            name + "_ms_max": round(float(ms.max()), 3)}


def forward(a, torch):
    from sushi_amd import track
    E, n = a.rows, a.shifts
    gen = torch.Generator(device="cuda").manual_seed(61)
    curves = torch.rand(E * n, dtype=torch.float32, device="cuda", generator=gen) * 0.5 + 0.25
    rows = [(e * n, 1.0) for e in range(E)]
    plain, ordered = track.TrackState(E, n, curves.device), track.TrackState(E, n, curves.device, ordered=True)
    for reach in (0, 88):
        run_plain = lambda: track.track_device(curves, rows, reach, PENALTY, 2.0 ** -12, plain)
        run_ordered = lambda: track.track_ordered_device(curves, rows, reach, PENALTY, 2.0 ** -12, BACK, ordered)
        run_free = lambda: track.track_ordered_device(curves, rows, reach, PENALTY, 2.0 ** -12, None, ordered)
        run_plain(), run_free()
        same = bool(torch.equal(plain.moves, ordered.moves) and torch.equal(plain.row_min.view(torch.int64), ordered.row_min.view(torch.int64)))
        run_ordered()
        ms = {"plain": [], "ordered": []}
        for _ in range(a.reps):
            ms["plain"].append(_wall(run_plain, torch)[0])
            ms["ordered"].append(_wall(run_ordered, torch)[0])
        out = {"case": "forward", "rows": E, "n_shift": n, "reach": reach, "back": BACK, "reps": a.reps,
               "without_a_limit_equals_plain": same}
        out.update(_stats(ms["plain"], "plain"))
        out.update(_stats(ms["ordered"], "ordered"))
        out["ordered_over_plain"] = round(out["ordered_ms"] / out["plain_ms"], 2)
        out["plain_us_per_row"] = round(out["plain_ms"] * 1e3 / E, 1)
        out["ordered_us_per_row"] = round(out["ordered_ms"] * 1e3 / E, 1)
        # bytes per (row, shift) from the code: the step moves 22 at reach 0 (D in 8, row 4, D out 8, move 2) and P in 8 more in
        # the ordered pass, whose prefix pass re-reads D (8) and writes P (8) and A (4)
        out["plain_GB_per_s"] = round(22.0 * E * n / out["plain_ms"] / 1e6, 1)
        out["ordered_GB_per_s"] = round(50.0 * E * n / out["ordered_ms"] / 1e6, 1)
        print(json.dumps(out), flush=True)
    del curves, plain, ordered
    torch.cuda.empty_cache()


def find(a, torch):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    seconds = a.hours * 3600.0
    dst_pcm = synth.make_dst_pcm(seconds, RATE, seed=51)
    src_pcm = synth.make_src_pcm(dst_pcm, int(OFFSET_S * RATE), seed=52)
    starts = np.linspace(200.0, seconds - 400.0, a.events)
    dst = WavStream.from_samples(dst_pcm, RATE, sample_type="uint8")
    src = WavStream.from_samples(src_pcm, RATE, sample_type="uint8")
    patterns = [src.get_substream(float(s), float(s) + EVENT_S) for s in starts]
    centres = [float(s) for s in starts]
    call = lambda **kw: dst.find_track(patterns, centres, WINDOW, PENALTY, reach=REACH, **kw)
    for method, clamp in (("sqdiff_normed", None), ("ccoeff_normed", None), ("ccoeff_normed", 0.5)):
        kw = dict(method=method) if clamp is None else dict(method=method, clamp=clamp)
        plain, ordered = call(**kw), call(order=True, **kw)                  # warm-up of both at this shape
        ms = {"plain": [], "ordered": []}
        for _ in range(a.reps):
            ms["plain"].append(_wall(lambda: call(**kw), torch)[0])
            ms["ordered"].append(_wall(lambda: call(order=True, **kw), torch)[0])
        out = {"case": "find_track", "sample_type": "uint8", "method": method, "clamp": clamp, "events": a.events,
               "n_shift": plain.n_shift, "reach": REACH, "reps": a.reps, "same_shifts": bool(plain.shifts == ordered.shifts),
               "found_offset_s": sorted(set(round(d, 4) for d in ordered.deltas))[:3]}
        out.update(_stats(ms["plain"], "plain"))
        out.update(_stats(ms["ordered"], "ordered"))
        out["ordered_over_plain"] = round(out["ordered_ms"] / out["plain_ms"], 3)
        print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--shifts", type=int, default=2880001)
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--skip-find", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_order_rate: needs a GPU (a rate is not measured on the CPU)")
    forward(a, torch)
    if not a.skip_find:
        find(a, torch)


if __name__ == "__main__":
    main()
