"""Rates of best-K runs (sushi_hip_batch_run_best) against the other routes to the same answer.  GPU.

Workload: tools/occurrence_rate.py's (DESIGN.md 3.10's table) -- 2 h destination stream at 12 kHz, 64 patterns of 3 s from a
separate source stream, each planted 1 to 3 times in the destination (gain 0.5 - 1, 0 - 20 dB of noise), every pattern searched
over the whole stream, TM_CCOEFF_NORMED, uint8 and float32 streams.  Separation: the pattern's own length.

  best-K run:      SearchBatch.run_best -- device time per run (HIP events, median of --reps), the block pairs evaluated exactly,
                   the last round that evaluated a pair of each search (1 the seed, 2 - 3 escalation, 4 the last stage);
  curve route:     match_curves of one request plus greedy suppression (not timed: the curve alone is the route's floor) -- device
                   time per pattern (median over --curve-patterns of them) x 64, as tools/occurrence_rate.py scales it;
  threshold route: (with a threshold only) SearchBatch.occurrences(threshold) + occurrences.peaks per request on the host, cut at K
                   -- wall time, what a caller had to do before; its device part (run_threshold) beside it.

Asks: K = 3 at threshold 0.6; K = 1, 2, 3 without a threshold.  Every best-K answer is checked against the threshold route's (with
a threshold) and, for the curve patterns timed, against best_peaks of the curve.  One JSON line per (dtype, K, threshold).
Usage: python tools/best_rate.py [--reps 3] [--curve-patterns 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from occurrence_rate import RATE, make_streams, time_it          # noqa: E402  (the same material)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--curve-patterns", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=7200.0)
    ap.add_argument("--dtypes", default="uint8,float32")
    ap.add_argument("--asks", default="3:0.6,1:,2:,3:", help="K:threshold, comma separated (no threshold: empty)")
    a = ap.parse_args()
    import torch
    from sushi_amd.curves import match_curves
    from sushi_amd.device import DeviceStream, SearchBatch
    from sushi_amd.occurrences import best_peaks, peaks
    n_pat, m = 64, 3 * RATE
    rows, planted = make_streams(a.seconds, n_pat, m, seed=5)
    asks = [(int(x.split(":")[0]), float(x.split(":")[1]) if x.split(":")[1] else None) for x in a.asks.split(",")]
    for dtype in a.dtypes.split(","):
        d_row, s_row = rows(dtype)
        dst, src = DeviceStream(d_row), DeviceStream(s_row)
        n = d_row.shape[0]
        P = n - m + 1
        offs = [k * m for k in range(n_pat)]
        b = SearchBatch(dst, src, offs, [m] * n_pat, [0] * n_pat, [P] * n_pat, path="fft", method="ccoeff_normed", exclusion="auto")
        out = torch.empty(P, dtype=torch.float32, device=dst.device)
        # the curve route's device time (the same for every ask), and the curves the answers are checked against
        cms, curves = [], {}
        for k in range(min(a.curve_patterns, n_pat)):
            cms.append(time_it(lambda: match_curves(dst, src, [offs[k]], [m], [0], [P], method="ccoeff_normed", out=out), 1)[0])
            curves[k] = out.cpu().numpy().copy()
        curve_ms = float(np.median(cms)) * n_pat if cms else float("nan")
        for K, thr in asks:
            res = {}

            def best_route():
                res["hits"], res["counts"] = b.run_best(K, None, thr)

            ms, ms_min = time_it(best_route, a.reps)
            d = b.diagnostics(per_search=True)
            rounds = np.bincount(np.asarray(d["flagged_per_search"], np.int64), minlength=5).tolist()
            h, cnt = res["hits"].cpu().numpy(), res["counts"].cpu().numpy()
            found = [(h[k, :int(cnt[k]), 0].astype(np.int64), np.ascontiguousarray(h[k, :int(cnt[k]), 1]).view(np.float32))
                     for k in range(n_pat)]
            for k, c in curves.items():
                wi, ws = best_peaks(c, K, m, "ccoeff_normed", threshold=thr)
                assert found[k][0].tolist() == wi.tolist() and found[k][1].view(np.uint32).tolist() == ws.view(np.uint32).tolist(), (dtype, K, thr, k)
            line = {
                "dtype": dtype, "method": "ccoeff_normed", "k": K, "threshold": thr, "searches": n_pat, "positions_per_search": P, "M": m,
                "best_ms": round(ms, 3), "best_ms_min": round(ms_min, 3), "pairs": int(b.fft_pairs),
                "pairs_evaluated": int(d["pairs_transformed"]), "share_evaluated": round(d["pairs_transformed"] / float(b.fft_pairs), 5),
                "band": int(d["band"]), "excluded_audited": int(d["excluded_audited"]), "slb_violations": int(d["slb_violations"]),
                "searches_by_last_round": rounds, "picks": int(sum(i.size for i, _ in found)),
                "planted": int(sum(len(c) for c in planted)),
                "planted_picked": sum(int(np.any(np.abs(found[k][0] - c) <= 2)) for k in range(n_pat) for c in planted[k]),
                "curve_route_ms": round(curve_ms, 2), "curve_route_patterns_timed": len(cms), "speedup_curve": round(curve_ms / ms, 2),
                "reps": a.reps}
            if thr is not None:
                # what a caller did before: all hits to the host, one peak per occurrence there, the best K of them
                def threshold_route():
                    res = []
                    for idx, sc in b.occurrences(thr):
                        pi, ps = peaks(idx, sc, m, "ccoeff_normed")
                        order = np.lexsort((pi, -ps.astype(np.float64)))[:K]
                        res.append((pi[order], ps[order]))
                    return res
                threshold_route()
                walls = []
                for _ in range(a.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    ref = threshold_route()
                    walls.append((time.perf_counter() - t0) * 1e3)
                for k in range(n_pat):
                    assert found[k][0].tolist() == ref[k][0].tolist() and \
                        found[k][1].view(np.uint32).tolist() == ref[k][1].view(np.uint32).tolist(), (dtype, K, thr, k)
                tms, _ = time_it(lambda: b.run_threshold(thr, 4096), a.reps)
                line.update({"threshold_route_wall_ms": round(float(np.median(walls)), 3), "threshold_run_ms": round(tms, 3),
                             "speedup_threshold_route": round(float(np.median(walls)) / ms, 2)})
            print(json.dumps(line), flush=True)
        del b


if __name__ == "__main__":
    main()
