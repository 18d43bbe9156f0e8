"""Rates of threshold runs (sushi_hip_batch_run_threshold) against the only other route to the same answer.  GPU.

Workload (BASELINE configs[2] size): 2 h destination stream at 12 kHz, 64 patterns of 3 s from a separate source stream, each
planted 1 to 3 times in the destination (gain 0.5 - 1, 0 - 20 dB of noise), every pattern searched over the whole stream (the
widest window: 64 x 3,516 block pairs), TM_CCOEFF_NORMED at thresholds 0.4 / 0.6 / 0.8, uint8 and float32 streams.

  threshold route: SearchBatch.run_threshold -- device time per run (HIP events, median), the share of block pairs evaluated
                   exactly (diagnostics pairs_transformed / fft_pairs), the hits;
  curve route:     match_curves of one request plus a device-side compare (torch: curve >= t, summed) -- device time per pattern
                   (median over the patterns timed) x 64.  A float32 curve of 86 M positions takes ~0.35 s: only
                   --curve-patterns of them are timed, and each one's count is checked against the threshold run's.

One JSON line per (dtype, threshold).  Usage: python tools/occurrence_rate.py [--reps 3] [--curve-patterns 8]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATE = 12000


def make_streams(seconds, n_pat, m, seed):
    """(rows(dtype) -> (dst row, src row), planted[k] = the samples where pattern k was planted)"""
    from sushi_amd import synth
    rng = np.random.default_rng(seed)
    src = synth.make_dst_pcm(n_pat * m / RATE + 1, RATE, seed=seed + 1).astype(np.float64)
    dst = synth.make_dst_pcm(seconds, RATE, seed=seed).astype(np.float64)
    n = dst.shape[0]
    slots = rng.permutation((n - m) // (2 * m))[: 3 * n_pat] * 2 * m      # places that do not overlap
    planted, s = [], 0
    for k in range(n_pat):
        pat = src[k * m:(k + 1) * m]
        p_sig = float(np.mean(pat ** 2))
        copies = []
        for _ in range(int(rng.integers(1, 4))):
            b, g, snr = int(slots[s]), float(rng.uniform(0.5, 1.0)), float(rng.uniform(0.0, 20.0))
            s += 1
            dst[b:b + m] = g * pat + rng.standard_normal(m) * np.sqrt(p_sig / 10.0 ** (snr / 10.0))
            copies.append(b)
        planted.append(copies)

    def row(x, dtype):
        x = ((x - x.min()) / (x.max() - x.min())).astype(np.float32)
        return (x * np.float32(255.0) + np.float32(0.5)).astype(np.uint8) if dtype == "uint8" else x
    return (lambda dtype: (row(dst, dtype), row(src, dtype))), planted


def time_it(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--curve-patterns", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=7200.0)
    ap.add_argument("--dtypes", default="uint8,float32")
    a = ap.parse_args()
    import torch
    from sushi_amd.curves import match_curves
    from sushi_amd.device import DeviceStream, SearchBatch
    n_pat, m = 64, 3 * RATE
    rows, planted = make_streams(a.seconds, n_pat, m, seed=5)
    for dtype in a.dtypes.split(","):
        d_row, s_row = rows(dtype)
        dst, src = DeviceStream(d_row), DeviceStream(s_row)
        n = d_row.shape[0]
        P = n - m + 1
        offs = [k * m for k in range(n_pat)]
        b = SearchBatch(dst, src, offs, [m] * n_pat, [0] * n_pat, [P] * n_pat, path="fft", method="ccoeff_normed", exclusion="auto")
        out = torch.empty(P, dtype=torch.float32, device=dst.device)
        for t in (0.4, 0.6, 0.8):
            res = {}

            def threshold_route():
                res["hits"], res["counts"] = b.run_threshold(t, 4096)

            def curve_route(k):
                match_curves(dst, src, [offs[k]], [m], [0], [P], method="ccoeff_normed", out=out)
                res["curve_count"] = (out >= t).sum()

            ms, ms_min = time_it(threshold_route, a.reps)
            d = b.diagnostics()
            counts = res["counts"].cpu().numpy()
            found = b.occurrences(t)
            copies_found = sum(int(np.any(np.abs(found[k][0] - c) <= 2)) for k in range(n_pat) for c in planted[k])
            cms = []
            for k in range(min(a.curve_patterns, n_pat)):
                cms.append(time_it(lambda: curve_route(k), 1)[0])
                assert int(res["curve_count"].item()) == int(counts[k]), (dtype, t, k, int(res["curve_count"].item()), int(counts[k]))
            curve_ms = float(np.median(cms)) * n_pat
            print(json.dumps({
                "dtype": dtype, "method": "ccoeff_normed", "threshold": t, "searches": n_pat, "positions_per_search": P, "M": m,
                "threshold_ms": round(ms, 3), "threshold_ms_min": round(ms_min, 3),
                "pairs": int(b.fft_pairs), "pairs_evaluated": int(d["pairs_transformed"]),
                "share_evaluated": round(d["pairs_transformed"] / float(b.fft_pairs), 5), "band": int(d["band"]),
                "excluded_audited": int(d["excluded_audited"]), "slb_violations": int(d["slb_violations"]),
                "hits": int(counts.sum()), "planted": int(sum(len(c) for c in planted)), "planted_found": copies_found,
                "curve_route_ms": round(curve_ms, 2), "curve_route_patterns_timed": len(cms),
                "speedup": round(curve_ms / ms, 2), "reps": a.reps}), flush=True)
        del b


if __name__ == "__main__":
    main()
