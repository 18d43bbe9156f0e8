"""Rate of sushi_hip_filter.  GPU.

A 2-h row at 12 kHz (86.4 M samples of body, 2 x 120,000 of padding, random samples, in_start = the padding), uint8 and float32,
T in {63, 255, 1023} random taps: device time per call (HIP events round --calls calls, two warm-up rounds, --reps repeats;
median, min, max), head and tail of the result checked against filter_host.  In the same process: a device copy of the row; the
same filter as torch expressions (conv1d in float64 on the centred row, 2^20 outputs a call, then the same finish; --no-baseline
skips it) and at how many positions its result is the kernel's; WavStream.filtered end to end on a loaded 2-h stream (host clock round a synchronise).

One JSON line per case.  Usage: python tools/filter_rate.py [--reps 7] [--calls 5] [--label NAME] [--no-baseline]
SUSHI_HIP_LIB picks an A/B build (-DSUSHI_FILTER_STRIDED: a thread owns outputs 256 apart).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BODY, PAD = 2 * 3600 * 12000, 120000
TORCH_CHUNK = 1 << 20        # outputs per conv1d call of the torch form (8.4 GB of float64 at 1023 taps if it unfolds)


def _times(fn, calls, reps):
    import torch
    for _ in range(2):
        for _ in range(calls):
            fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / calls)
    return {"ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}


def _row(dtype):
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    n = BODY + 2 * PAD
    if dtype == "uint8":
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    return torch.rand(n, dtype=torch.float32, device="cuda", generator=g)


def _taps(n_taps):
    h = np.random.default_rng(n_taps).standard_normal(n_taps)
    return h / np.abs(h).sum()


def _torch_form(x, h_dev, n_taps):
    """The same filter as torch expressions: conv1d (a correlation) in float64 on the centred row, the same finish."""
    import torch
    a = (n_taps - 1) // 2
    u8 = x.dtype == torch.uint8
    out = torch.empty(BODY, dtype=x.dtype, device=x.device)
    for i0 in range(0, BODY, TORCH_CHUNK):                       # in chunks: a float64 convolution may unfold its input, T doubles an output
        m = min(TORCH_CHUNK, BODY - i0)
        d = x[PAD + i0 - a:PAD + i0 + m + a].to(torch.float64) - (128.0 if u8 else 0.5)
        acc = torch.nn.functional.conv1d(d.view(1, 1, -1), h_dev.view(1, 1, -1)).view(-1)
        out[i0:i0 + m] = torch.floor(acc + 128.5).clamp(0.0, 255.0).to(torch.uint8) if u8 else (acc + 0.5).to(torch.float32)
    return out


def kernel_cases(dtype, a):
    import torch
    from sushi_amd import _native, filter as F
    L = _native.lib()
    x = _row(dtype)
    out = torch.empty(BODY, dtype=x.dtype, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    code = _native.U8 if dtype == "uint8" else _native.F32
    size = x.element_size()
    n = int(x.shape[0])
    y = torch.empty_like(x)
    rec = {"what": "copy", "sample_type": dtype, "bytes": 2 * n * size}
    rec.update(_times(lambda: y.copy_(x), a.calls, a.reps))
    rec["TB_per_s"] = rec["bytes"] / (rec["ms_median"] * 1e-3) / 1e12
    yield rec
    del y
    for n_taps in (63, 255, 1023):
        h = _taps(n_taps)
        h_dev = torch.from_numpy(h).cuda()

        def call():
            rc = L.sushi_hip_filter(x.data_ptr(), code, n, PAD, h_dev.data_ptr(), n_taps, out.data_ptr(), BODY, st)
            assert rc == 0, rc

        rec = {"what": "kernel", "label": a.label, "sample_type": dtype, "n_taps": n_taps, "samples": BODY, "bytes": 2 * BODY * size}
        rec.update(_times(call, a.calls, a.reps))
        rec["TB_per_s"] = rec["bytes"] / (rec["ms_median"] * 1e-3) / 1e12
        rec["G_taps_per_s"] = BODY * n_taps / (rec["ms_median"] * 1e-3) / 1e9      # products, and as many additions
        # the result is the restatement's: head (reads the left pad) and tail (reads the right pad)
        m = 1 << 16
        xs = x.cpu().numpy()
        got = out.cpu().numpy()
        assert got[:m].tobytes() == F.filter_host(xs, PAD, h, m).tobytes()
        assert got[-m:].tobytes() == F.filter_host(xs, PAD + BODY - m, h, m).tobytes()
        yield rec
        if a.no_baseline:
            continue
        rec = {"what": "torch", "sample_type": dtype, "n_taps": n_taps, "samples": BODY}
        try:
            t0 = time.perf_counter()
            ref = _torch_form(x, h_dev, n_taps)
            torch.cuda.synchronize()
            first = time.perf_counter() - t0
            rec["first_call_s"] = first
            reps = a.reps if first < 0.5 else (3 if first < 5.0 else 1)
            rec.update(_times(lambda: _torch_form(x, h_dev, n_taps), 1, reps) if first < 30.0 else
                       {"ms_median": first * 1e3, "ms_min": first * 1e3, "ms_max": first * 1e3})
            rec["equal_positions"] = int((ref == out).sum().item())
            del ref
        except Exception as e:                                   # (no float64 convolution in this build, or no memory for it)
            rec["error"] = "%s: %s" % (type(e).__name__, str(e)[:200])
        torch.cuda.empty_cache()
        yield rec


def stream_cases(dtype, a):
    """WavStream.filtered end to end: the launch, fill_pads and the copy of the new row to the host for .data."""
    import torch
    from sushi_amd.wav import WavStream
    x = _row(dtype)
    w = WavStream.from_prepared(x.cpu().numpy().reshape(1, -1), 12000, BODY, PAD)
    w._dev_row = x                                               # as a loaded stream holds it: the row already in HBM
    for kw in ({"low": 150}, {"low": 150, "n_taps": 1023}):
        ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = w.filtered(**kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            del f
        yield {"what": "WavStream.filtered", "label": a.label, "sample_type": dtype, "args": kw, "samples": BODY,
               "host_bytes": int(x.shape[0]) * x.element_size(), "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)),
               "ms_max": float(np.max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--label", default="as shipped")
    ap.add_argument("--no-baseline", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("filter_rate.py measures on the GPU: none is visible")
    for dtype in ("uint8", "float32"):
        for rec in kernel_cases(dtype, a):
            print(json.dumps(rec), flush=True)
        if not a.no_baseline:
            for rec in stream_cases(dtype, a):
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
