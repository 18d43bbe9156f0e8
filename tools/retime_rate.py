"""Rate of sushi_hip_retime.  GPU.

  (a) a 2-h stream (86.4 M samples at 12 kHz), uint8 and float32, read at step 24 / 25 (a source that plays 25/24 fast put on the
      destination's clock: 90 M outputs) -- device time per call (HIP events, median of --reps runs after a warm-up), against a
      device-to-device copy of the same input-plus-output bytes in the same process;
  (b) estimate_speed at the size of the end-to-end test (a 150 s destination, a source at 25/24, 4 probes, the 7 standard
      candidates): wall time of the call, first and later ones.

One JSON line per case.  Usage: python tools/retime_rate.py [--reps 20]
"""
import argparse
import json
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps):
    import torch
    for _ in range(3):
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


def kernel_case(dtype, reps):
    import torch
    from sushi_amd import retime
    n_in = 2 * 3600 * 12000
    num, den = 24, 25
    n_out = (n_in - 1) * den // num + 1
    g = torch.Generator(device="cuda").manual_seed(5)
    if dtype == "uint8":
        x = torch.randint(0, 256, (n_in,), dtype=torch.uint8, device="cuda", generator=g)
    else:
        x = torch.rand(n_in, dtype=torch.float32, device="cuda", generator=g)
    out = torch.empty(n_out, dtype=x.dtype, device="cuda")
    seg = np.array([(0, 0, n_out, num, den)], dtype=retime._native.RETIME_SEGMENT_DTYPE)
    size = x.element_size()
    nbytes = (n_in + n_out) * size
    # a copy that moves as many bytes: reads (n_in + n_out) / 2 samples and writes as many
    half = (n_in + n_out) // 2
    a_buf, b_buf = torch.empty(half, dtype=x.dtype, device="cuda"), torch.empty(half, dtype=x.dtype, device="cuda")
    a_buf[:n_in].copy_(x)
    a_buf[n_in:].copy_(x[:half - n_in])
    # the table and the workspace are prepared once: the events bracket the library call alone (argument checks, the 48-byte
    # upload of the table, the launch), not retime_device's NumPy checks and allocation
    L = retime._native.lib()
    mem = torch.empty(max(256, L.sushi_hip_retime_bytes(1)), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    code = retime._native.U8 if dtype == "uint8" else retime._native.F32

    def call():
        rc = L.sushi_hip_retime(x.data_ptr(), code, n_in, seg.ctypes.data, 1, out.data_ptr(), n_out, mem.data_ptr(), mem.numel(), st)
        assert rc == 0, rc

    def four_calls():
        for _ in range(4):
            call()

    t_k, t_k_min = _median_ms(call, reps)
    t_k4, _ = _median_ms(four_calls, reps)                   # back to back: what is left of the host's share per call
    t_c, t_c_min = _median_ms(lambda: b_buf.copy_(a_buf), reps)
    t_w, _ = _median_ms(lambda: retime.retime_device(x, seg, out=out), reps)      # the Python wrapper, checks and allocation included
    # the result is the restatement's (a slice of it: the whole stream takes NumPy a while)
    m = 1 << 20
    want_head = retime.retime_host(x[:m + 2].cpu().numpy(), [(0, 0, m, num, den)])
    assert out[:m].cpu().numpy().tobytes() == want_head.tobytes()
    i0 = (n_out - m) // den * den                              # an output that reads a whole input sample: a segment can start there
    want_tail = retime.retime_host(x[i0 * num // den:].cpu().numpy(), [(0, 0, n_out - i0, num, den)])
    assert out[i0:].cpu().numpy().tobytes() == want_tail.tobytes()
    return {"case": "retime_2h", "dtype": dtype, "n_in": n_in, "n_out": n_out, "step": "%d/%d" % (num, den), "bytes": nbytes,
            "ms": round(t_k, 4), "ms_min": round(t_k_min, 4), "gb_per_s": round(nbytes / (t_k * 1e-3) / 1e9, 1),
            "copy_ms": round(t_c, 4), "copy_ms_min": round(t_c_min, 4), "copy_gb_per_s": round(2 * half * size / (t_c * 1e-3) / 1e9, 1),
            "ratio_to_copy": round(t_k / t_c, 3), "ms_per_call_of_four_back_to_back": round(t_k4 / 4, 4),
            "wrapper_ms": round(t_w, 4), "outputs_per_s": n_out / (t_k * 1e-3), "reps": reps}


def estimate_case():
    from sushi_amd import retime, synth
    from sushi_amd.wav import WavStream
    rate, speed = 12000, Fraction(25, 24)
    dst_pcm = synth.make_dst_pcm(150, rate, seed=3)
    first = 5 * rate
    n_src = ((dst_pcm.shape[0] - 2 - first) * speed.denominator) // speed.numerator + 1
    t = first * speed.denominator + np.arange(n_src, dtype=np.int64) * speed.numerator
    j, r = t // speed.denominator, t % speed.denominator
    x = dst_pcm.astype(np.float64)
    y = x[j] + (r / float(speed.denominator)) * (x[j + 1] - x[j])
    y += np.random.default_rng(1).standard_normal(n_src) * np.sqrt(np.mean(x ** 2) / 100.0)
    src_pcm = np.clip(np.round(y), -32768, 32767).astype(np.int16)
    dst = WavStream.from_samples(dst_pcm, rate, sample_type="uint8")
    src = WavStream.from_samples(src_pcm, rate, sample_type="uint8")
    walls = [retime.estimate_speed(src, dst, probes=4) for _ in range(5)]
    return {"case": "estimate_speed", "dtype": "uint8", "dst_seconds": 150, "probes": 4, "candidates": len(retime.STANDARD_SPEEDS),
            "speed": str(walls[-1].speed), "fitted": walls[-1].fitted, "offset_seconds": walls[-1].offset_seconds,
            "first_call_ms": round(walls[0].seconds * 1e3, 2), "later_calls_ms": round(float(np.median([w.seconds for w in walls[1:]])) * 1e3, 2),
            "includes": "the streams' first trip to HBM and the destination's spectra (first call), retime launch, batch set-up, run, D2H"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("retime_rate.py measures on the GPU: none is visible")
    for dtype in ("uint8", "float32"):
        print(json.dumps(kernel_case(dtype, max(20, a.reps))), flush=True)
    print(json.dumps(estimate_case()), flush=True)


if __name__ == "__main__":
    main()
