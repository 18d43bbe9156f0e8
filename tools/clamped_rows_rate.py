"""What clamping the score rows of a shift-axis search buys (clamp=).  GPU.

find_track and find_segments on 64 events of 3 s cut from a 2-h 12 kHz source that is the destination advanced by 30 s, +-120 s
windows (n_shift = 2,880,001), in uint8 and float32 streams: 'ccoeff_normed' at clamp 0.5 and 0.3, 'sqdiff_normed' at 0.2 (as many
hits as at coefficient 0.5), each against the unclamped call -- whole calls, host clock around a device synchronise, by turns in one process, median
of --reps runs after a warm-up.  The unclamped call is the code of the commit before clamp= existed; --tree DIR times it from
another checkout (that commit's) with --unclamped-only, for a comparison in the same session.

Per case one JSON line: both times and their ratio, rows_info (requests formed from hits / densely, hits, block pairs the threshold
run evaluated exactly), whether the clamped call's shifts equal the unclamped call's, and the split of one clamped forming into
batch set-up, threshold run, fill and scatter (with the read of the flags), and the pass.
Usage: python tools/clamped_rows_rate.py [--reps 5] [--events 64] [--hours 2] [--unclamped-only] [--tree DIR]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

RATE, EVENT_S, WINDOW, OFFSET_S = 12000, 3.0, 120.0, 30.0
PENALTY, REACH = 0.5, 16
# (in these streams a peak falls by about 0.12 a sample in the coefficient and rises by 0.05 a sample in TM_SQDIFF_NORMED, whose chance
# level is 0.41: coefficient 0.5 and TM_SQDIFF_NORMED 0.2 both keep seven positions of a peak, coefficient 0.3 eleven)
CASES = [("ccoeff_normed", 0.5), ("ccoeff_normed", 0.3), ("sqdiff_normed", 0.2)]


def _wall(fn, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _split(dst, patterns, centres, method, clamp, torch):
    """One forming of the clamped rows and one tracking pass over them, stage by stage (milliseconds, host clock, a synchronise
    after each)."""
    from sushi_amd import axis, rows, track
    from sushi_amd.device import SearchBatch
    dst_dev = dst.device_stream()
    src_dev, offs, lens, _ = dst._pattern_source(patterns, dst_dev)
    ax = axis.event_axis(dst, offs, axis.pattern_lengths(lens), centres, WINDOW)
    E, n = len(patterns), ax.n_shift
    f = axis.clamp_value(clamp, method)
    cap = axis.default_capacity(E, n)
    starts = [b + ax.k_lo for b in ax.bases]
    ms = {}
    ms["batch_setup"], batch = _wall(lambda: SearchBatch(dst_dev, src_dev, ax.offs, ax.lens, starts, [n] * E, path="fft", method=method), torch)
    ms["threshold_run"], (hits, counts) = _wall(lambda: batch.run_threshold(float(f), cap), torch)
    curves = torch.empty(E * n, dtype=torch.float32, device=dst_dev.device)
    table = rows.rows_table(np.arange(E, dtype=np.int64) * n, [n] * E)
    ms["fill_scatter"], flags = _wall(lambda: rows.rows_from_hits_device(hits, counts, table, f, curves).cpu().numpy(), torch)
    state = track.TrackState(E, n, dst_dev.device)

    def run_pass():
        track.track_device(curves, [(e * n, 1.0) for e in range(E)], [0] + [REACH] * (E - 1), PENALTY, 0.0, state, method=method)
        return track.track_backtrack_device(state)

    ms["pass"], _ = _wall(run_pass, torch)
    ms = {k: round(v, 3) for k, v in ms.items()}
    ms["overflowed"] = int((flags & rows.OVERFLOW).sum())
    ms["fill_GB_per_s"] = round(4.0 * E * n / ms["fill_scatter"] / 1e6, 1)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--events", type=int, default=64)
    ap.add_argument("--hours", type=float, default=2.0)
    ap.add_argument("--unclamped-only", action="store_true")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("clamped_rows_rate: needs a GPU (a rate is not measured on the CPU)")
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    seconds = a.hours * 3600.0
    dst_pcm = synth.make_dst_pcm(seconds, RATE, seed=51)
    src_pcm = synth.make_src_pcm(dst_pcm, int(OFFSET_S * RATE), seed=52)
    starts = np.linspace(200.0, seconds - 400.0, a.events)
    for sample_type in ("uint8", "float32"):
        dst = WavStream.from_samples(dst_pcm, RATE, sample_type=sample_type)
        src = WavStream.from_samples(src_pcm, RATE, sample_type=sample_type)
        patterns = [src.get_substream(float(s), float(s) + EVENT_S) for s in starts]
        centres = [float(s) for s in starts]
        searches = {
            "find_track": lambda **kw: dst.find_track(patterns, centres, WINDOW, PENALTY, reach=REACH, **kw),
            "find_segments": lambda **kw: dst.find_segments(patterns, centres, WINDOW, PENALTY, **kw)}
        for method, clamp in ([(m, None) for m in dict(CASES)] if a.unclamped_only else CASES):
            for name, call in searches.items():
                plain = call(method=method)                                     # warm-up of both at this shape
                if not a.unclamped_only:
                    clamped = call(method=method, clamp=clamp)
                ms = {"unclamped": [], "clamped": []}
                for _ in range(a.reps):
                    ms["unclamped"].append(_wall(lambda: call(method=method), torch)[0])
                    if not a.unclamped_only:
                        ms["clamped"].append(_wall(lambda: call(method=method, clamp=clamp), torch)[0])
                out = {"search": name, "sample_type": sample_type, "method": method, "events": a.events, "n_shift": plain.n_shift,
                       "reps": a.reps, "tree": os.path.relpath(os.path.abspath(a.tree)),
                       "unclamped_ms": round(float(np.median(ms["unclamped"])), 2), "unclamped_ms_min": round(float(np.min(ms["unclamped"])), 2),
                       "found_offset_s": sorted(set(round(d, 4) for d in plain.deltas))[:3]}
                if not a.unclamped_only:
                    out.update({"clamp": clamp, "f": clamped.clamp, "clamped_ms": round(float(np.median(ms["clamped"])), 2),
                                "clamped_ms_min": round(float(np.min(ms["clamped"])), 2),
                                "unclamped_over_clamped": round(float(np.median(ms["unclamped"]) / np.median(ms["clamped"])), 2),
                                "rows_info": clamped.rows_info, "same_shifts": bool(clamped.shifts == plain.shifts)})
                    if name == "find_track":
                        out["split_ms"] = _split(dst, patterns, centres, method, clamp, torch)
                print(json.dumps(out), flush=True)
        del dst, src, patterns
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
