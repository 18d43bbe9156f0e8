"""What the margins of the ordered pass cost (find_ordered_track(margins=True)).  GPU.

Passes: on random float32 rows -- 64 rows of 2,880,001 shifts at every reach 0 and every reach 88, 200 rows of 240,001 shifts at
reach 16, backs of 36,000 shifts, a guard of 120 -- sushi_hip_track_forward_ordered, sushi_hip_track_forward_ordered_keep and
sushi_hip_track_order_margins with and without M_dev, by turns in one process, HIP events around each call, median of --reps
runs after a warm-up, with the spread.  The forward pass is three launches per row, and so is the margins call.

The same backward pass as torch expressions on the kept rows (flip + cummin for the suffix minimum, one shifted minimum per
candidate of the window), timed the same way with fewer repetitions; its best, alt and through are compared with the call's bit
for bit.

End to end: find_ordered_track with and without margins=True on 64 events of 3 s cut from a 2-h 12 kHz uint8 source that is the
destination advanced by 30 s, +-120 s windows (the same n_shift), reach 16, order=True: whole calls, a host clock around a device
synchronise.

--only margins runs the margins call alone a few times at the first shape: what a kernel trace of its own is taken from;
--only find runs the end-to-end case alone.

One JSON line per case.
Usage: python tools/track_order_margins_rate.py [--reps 7] [--torch-reps 2] [--events 64] [--hours 2] [--skip-find] [--only margins|find]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

RATE, EVENT_S, WINDOW, OFFSET_S = 12000, 3.0, 120.0, 30.0
PENALTY, STEP_COST, BACK, GUARD = 0.5, 2.0 ** -12, 36000, 120
SHAPES = ((64, 2880001, 0), (64, 2880001, 88), (200, 240001, 16))        # (rows, shifts, reach)


def _event_ms(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


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


def torch_margins(curves, E, n, reach, D, shifts, torch):
    """The backward pass of the ordered margins as torch expressions (weights 1, 'sqdiff_normed', one penalty, one back, one
    guard): (through, best, best_arg, alt, alt_arg), float64 / int64 tensors of E."""
    j = torch.arange(n, device=curves.device)
    at = torch.clamp(j - BACK, min=0)
    inf = torch.tensor(float("inf"), dtype=torch.float64, device=curves.device)
    through, best, best_arg, alt, alt_arg = [], [], [], [], []
    C = None
    for e in range(E - 1, -1, -1):
        u = curves[e * n:(e + 1) * n].double()
        if e == E - 1:
            M, C = D[e], u
        else:
            S = torch.flip(torch.cummin(torch.flip(C, (0,)), 0).values, (0,))
            jump = S[at] + PENALTY
            near = C.clone()
            for a in range(1, reach + 1):
                price = STEP_COST * float(a)
                near[a:] = torch.minimum(near[a:], C[:n - a] + price)
                near[:n - a] = torch.minimum(near[:n - a], C[a:] + price)
            B = torch.where(near <= jump, near, jump)
            M, C = D[e] + B, u + B
        s = shifts[e]
        through.append(M[s])
        m, k = torch.min(M, 0)
        best.append(m), best_arg.append(k)
        m, k = torch.min(torch.where((j - s).abs() > GUARD, M, inf), 0)
        alt.append(m), alt_arg.append(k)
    stack = lambda v: torch.stack(v[::-1])
    return stack(through), stack(best), stack(best_arg), stack(alt), stack(alt_arg)


def passes(a, torch, only_margins=False):
    from sushi_amd import track
    for E, n, reach in SHAPES[:1] if only_margins else SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(61)
        curves = torch.rand(E * n, dtype=torch.float32, device="cuda", generator=gen) * 0.5 + 0.25
        rows = [(e * n, 1.0) for e in range(E)]
        plain = track.TrackState(E, n, curves.device, ordered=True)
        kept = track.TrackState(E, n, curves.device, ordered=True, margins=True)
        M = torch.empty(E * n, dtype=torch.float64, device="cuda")
        run_forward = lambda: track.track_ordered_device(curves, rows, reach, PENALTY, STEP_COST, BACK, plain)
        run_keep = lambda: track.track_ordered_keep_device(curves, rows, reach, PENALTY, STEP_COST, BACK, kept)
        run_forward(), run_keep()
        shifts = track.track_ordered_backtrack_device(kept)
        margins = lambda m: track.track_ordered_margins_device(curves, rows, reach, GUARD, PENALTY, STEP_COST, BACK, kept, shifts,
                                                               marginals=m)
        margins(M), margins(None)
        if only_margins:
            for _ in range(3):
                margins(None)
            torch.cuda.synchronize()
            return
        same_forward = bool(torch.equal(plain.moves, kept.moves) and torch.equal(plain.row_min.view(torch.int64), kept.row_min.view(torch.int64))
                            and torch.equal(plain.last_D().view(torch.int64), kept.last_D().view(torch.int64)))
        ms = {"forward": [], "keep": [], "margins": [], "margins_M": []}
        for _ in range(a.reps):
            ms["forward"].append(_event_ms(run_forward, torch)[0])
            ms["keep"].append(_event_ms(run_keep, torch)[0])
            ms["margins"].append(_event_ms(lambda: margins(None), torch)[0])
            ms["margins_M"].append(_event_ms(lambda: margins(M), torch)[0])
        D = kept.D.view(E, n)
        t_ms, want = [], None
        torch_margins(curves, min(E, 2), n, reach, D, shifts, torch)           # warm-up
        for _ in range(a.torch_reps):
            t, want = _event_ms(lambda: torch_margins(curves, E, n, reach, D, shifts, torch), torch)
            t_ms.append(t)
        same_torch = bool(torch.equal(want[0].view(torch.int64), kept.through.view(torch.int64))
                          and torch.equal(want[1].view(torch.int64), kept.best.view(torch.int64))
                          and torch.equal(want[2].int(), kept.best_arg)
                          and torch.equal(want[3].view(torch.int64), kept.alt.view(torch.int64))
                          and torch.equal(want[4].int(), kept.alt_arg))
        out = {"case": "passes", "rows": E, "n_shift": n, "reach": reach, "back": BACK, "guard": GUARD, "reps": a.reps,
               "torch_reps": a.torch_reps, "keep_equals_forward": same_forward, "torch_equals_call_bitwise": same_torch}
        for name in ("forward", "keep", "margins", "margins_M"):
            out.update(_stats(ms[name], name))
        out.update(_stats(t_ms, "torch"))
        out["keep_over_forward"] = round(out["keep_ms"] / out["forward_ms"], 3)
        out["margins_over_forward"] = round(out["margins_ms"] / out["forward_ms"], 3)
        out["margins_M_over_forward"] = round(out["margins_M_ms"] / out["forward_ms"], 3)
        out["torch_over_margins"] = round(out["torch_ms"] / out["margins_ms"], 1)
        out["forward_us_per_row"] = round(out["forward_ms"] * 1e3 / E, 1)
        out["margins_us_per_row"] = round(out["margins_ms"] * 1e3 / E, 1)
        # bytes per (row, shift) from the code at reach 0: the step reads C 8, S 8, D 8 and the row 4 and writes C 8 (and M 8); the
        # apply re-reads C 8 and writes S 8
        out["margins_GB_per_s"] = round(52.0 * E * n / out["margins_ms"] / 1e6, 1)
        print(json.dumps(out), flush=True)
        del curves, plain, kept, M, D, want
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
    # (the kept rows of 64 events at +-120 s are 2.5 GiB, above find_ordered_track's default max_state_bytes of 2 GiB)
    call = lambda **kw: dst.find_ordered_track(patterns, centres, WINDOW, PENALTY, order=True, reach=16, max_state_bytes=4 << 30, **kw)
    off, on = call(), call(margins=True)                                       # warm-up of both at this shape
    ms = {"off": [], "on": []}
    for _ in range(a.reps):
        ms["off"].append(_wall(lambda: call(), torch)[0])
        ms["on"].append(_wall(lambda: call(margins=True), torch)[0])
    out = {"case": "find_ordered_track", "sample_type": "uint8", "method": "sqdiff_normed", "events": a.events, "n_shift": off.n_shift,
           "reach": 16, "reps": a.reps, "same_shifts": bool(off.shifts == on.shifts),
           "found_offset_s": sorted(set(round(d, 4) for d in on.deltas))[:3],
           "smallest_margin": float(np.min(on.event_margin)), "largest_margin": float(np.max(on.event_margin))}
    out.update(_stats(ms["off"], "without_margins"))
    out.update(_stats(ms["on"], "with_margins"))
    out["with_over_without"] = round(out["with_margins_ms"] / out["without_margins_ms"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--skip-find", action="store_true")
    ap.add_argument("--only", choices=["margins", "find"])
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("track_order_margins_rate: needs a GPU (a rate is not measured on the CPU)")
    if a.only != "find":
        passes(a, torch, only_margins=a.only == "margins")
    if not a.skip_find and a.only != "margins":
        find(a, torch)


if __name__ == "__main__":
    main()
