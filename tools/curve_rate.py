"""Rates of the whole-curve entry point (sushi_hip_match_curves; DESIGN.md "Curves").  GPU.

  (a) BASELINE configs[2] size: one curve of P = 2,880,001 positions (+-120 s at 12 kHz) and M = 36,000 (a 3 s pattern),
      uint8 and float32 streams, both methods -- device time per call (HIP events), MAC/s and the fraction of the peak of
      the pipe it runs on (uint8: dense i8 MFMA, ~5.0e15 ops/s = 2.5e15 MAC/s; float32: FP64 vector FMA, 78.6 TFLOP/s =
      3.93e13 FMA/s);
  (b) a drop-in WavStream.match_template call at Sushi's default window (+-10 s, 3 s pattern): wall time per call, D2H of the
      row included.

One JSON line per case.  Usage: python tools/curve_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_MAC = {"uint8": 2.5e15, "float32": 78.6e12 / 2}


def device_case(dtype, method, reps):
    import torch
    from sushi_amd.curves import match_curves
    from sushi_amd.device import DeviceStream
    rng = np.random.default_rng(7)
    P, M = 2880001, 36000
    n = P + M + 4096
    if dtype == "uint8":
        row = rng.integers(0, 256, n, dtype=np.uint8)
    else:
        row = (rng.standard_normal(n) * 0.2 + 0.5).clip(0, 1).astype(np.float32)
    dst = DeviceStream(row)
    out = torch.empty(P, dtype=torch.float32, device=dst.device)
    args = (dst, dst, [1000], [M], [2048], [P])
    match_curves(*args, method=method, out=out)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        match_curves(*args, method=method, out=out)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    t = float(np.median(ms))
    macs = float(P) * M
    rate = macs / (t * 1e-3)
    return {"case": "configs2_curve", "dtype": dtype, "method": method, "P": P, "M": M, "ms": round(t, 4),
            "ms_min": round(float(np.min(ms)), 4), "mac_per_s": rate, "peak_mac_per_s": PEAK_MAC[dtype],
            "peak_fraction": round(rate / PEAK_MAC[dtype], 4), "reps": reps}


def dropin_case(sample_type, reps):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    rate, seconds, off = 12000, 600.0, 2.5
    dst_pcm = synth.make_dst_pcm(seconds, rate, seed=1)
    src_pcm = synth.make_src_pcm(dst_pcm, int(off * rate), seed=2)
    dws = WavStream.from_samples(dst_pcm, rate, sample_rate=rate, sample_type=sample_type)
    sws = WavStream.from_samples(src_pcm, rate, sample_rate=rate, sample_type=sample_type)
    pat = sws.get_substream(300.0, 303.0)
    r = dws.match_template(pat, 300.0 + off, 10.0)          # first call: streams to HBM, code object
    walls = []
    for k in range(reps):
        t0 = time.perf_counter()
        r = dws.match_template(pat, 300.0 + off + 0.01 * k, 10.0)
        walls.append((time.perf_counter() - t0) * 1e3)
    P, M = r.shape[1], pat.shape[1]
    t = float(np.median(walls))
    return {"case": "dropin_match_template", "dtype": sample_type, "method": "sqdiff_normed", "P": P, "M": M,
            "ms": round(t, 4), "ms_min": round(float(np.min(walls)), 4), "mac_per_s": float(P) * M / (t * 1e-3),
            "peak_mac_per_s": PEAK_MAC[sample_type], "peak_fraction": round(float(P) * M / (t * 1e-3) / PEAK_MAC[sample_type], 5),
            "includes": "window arithmetic, launch, D2H of the row", "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    for dtype in ("uint8", "float32"):
        for method in ("sqdiff_normed", "ccoeff_normed"):
            print(json.dumps(device_case(dtype, method, a.reps)), flush=True)
    for st in ("uint8", "float32"):
        print(json.dumps(dropin_case(st, a.reps)), flush=True)


if __name__ == "__main__":
    main()
