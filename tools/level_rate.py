"""Rate of sushi_hip_level.  GPU.

A 2-h row at 12 kHz (86.4 M samples of body, 2 x 120,000 of padding, random samples, in_start = the padding), uint8 and float32,
W in {33, 129, 1023}.  Per sample type, in one process and interleaved -- every repeat times every case once, in turn: a device
copy of the row; sushi_hip_level at each W; sushi_hip_filter at n_taps = W (random taps); the same levelling as torch expressions
(float64 abs, conv1d with ones, then the divisions; 2^20 outputs a call; --no-baseline skips it).  Device time per call (HIP
events round --calls calls; two warm-up rounds of every case first; --reps repeats; median, min, max).  Before the timing the
head and tail of every levelled row are checked against level_host, and the torch form is compared with the kernel's result.
Then WavStream.levelled end to end on a loaded 2-h stream (host clock round a synchronise).

One JSON line per case.  Usage: python tools/level_rate.py [--reps 7] [--calls 5] [--label NAME] [--no-baseline]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BODY, PAD = 2 * 3600 * 12000, 120000
WINDOWS = (33, 129, 1023)
FLOOR, PEAK = 1.0 / 128, 8.0
TORCH_CHUNK = 1 << 20        # outputs per conv1d call of the torch form (a float64 convolution may unfold its input)


def _row(dtype):
    import torch
    g = torch.Generator(device="cuda").manual_seed(5)
    n = BODY + 2 * PAD
    if dtype == "uint8":
        return torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    return torch.rand(n, dtype=torch.float32, device="cuda", generator=g)


def _torch_form(x, ones, window):
    """The same levelling as torch expressions; the window sum is conv1d's, in whatever order it sums."""
    import torch
    h = (window - 1) // 2
    u8 = x.dtype == torch.uint8
    centre, half = (128.0, 128.0) if u8 else (0.5, 0.5)
    fw = (FLOOR * half) * float(window)
    out = torch.empty(BODY, dtype=x.dtype, device=x.device)
    for i0 in range(0, BODY, TORCH_CHUNK):
        m = min(TORCH_CHUNK, BODY - i0)
        d = x[PAD + i0 - h:PAD + i0 + m + h].to(torch.float64) - centre
        e = torch.nn.functional.conv1d(d.abs().view(1, 1, -1), ones.view(1, 1, -1)).view(-1)
        q = torch.nan_to_num((d[h:h + m] * float(window)) / ((e + fw) * PEAK), nan=0.0).clamp(-1.0, 1.0)
        out[i0:i0 + m] = torch.floor(q * 128.0 + 128.5).clamp(max=255.0).to(torch.uint8) if u8 else (0.5 + 0.5 * q).to(torch.float32)
    return out


def _interleaved(cases, reps):
    """cases: (record, fn, calls).  Two warm-up rounds of every case, then `reps` repeats that time every case once, in turn."""
    import torch
    for _ in range(2):
        for _rec, fn, calls in cases:
            for _ in range(calls):
                fn()
    torch.cuda.synchronize()
    ms = [[] for _ in cases]
    for _ in range(reps):
        for k, (_rec, fn, calls) in enumerate(cases):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / calls)
    for (rec, _fn, _calls), m in zip(cases, ms):
        rec.update({"ms_median": float(np.median(m)), "ms_min": float(np.min(m)), "ms_max": float(np.max(m)), "reps": reps})
        yield rec


def kernel_cases(dtype, a):
    import torch
    from sushi_amd import _native, level as LV
    L = _native.lib()
    x = _row(dtype)
    xs = x.cpu().numpy()
    out = torch.empty(BODY, dtype=x.dtype, device="cuda")
    y = torch.empty_like(x)
    st = torch.cuda.current_stream().cuda_stream
    code = _native.U8 if dtype == "uint8" else _native.F32
    size, n = x.element_size(), int(x.shape[0])
    cases = [({"what": "copy", "sample_type": dtype, "bytes": 2 * n * size}, lambda: y.copy_(x), a.calls)]
    for window in WINDOWS:
        def level(window=window):
            rc = L.sushi_hip_level(x.data_ptr(), code, n, PAD, window, FLOOR, PEAK, out.data_ptr(), BODY, st)
            assert rc == 0, rc

        # the result is the restatement's: head (reads the left pad) and tail (reads the right pad)
        level()
        got = out.cpu().numpy()
        m = 1 << 16
        assert got[:m].tobytes() == LV.level_host(xs, PAD, window, FLOOR, PEAK, m).tobytes()
        assert got[-m:].tobytes() == LV.level_host(xs, PAD + BODY - m, window, FLOOR, PEAK, m).tobytes()
        rec = {"what": "level", "label": a.label, "sample_type": dtype, "window": window, "samples": BODY, "bytes": 2 * BODY * size}
        if not a.no_baseline:
            ones = torch.ones(window, dtype=torch.float64, device="cuda")
            try:
                t0 = time.perf_counter()
                ref = _torch_form(x, ones, window)
                torch.cuda.synchronize()
                first = time.perf_counter() - t0
                trec = {"what": "torch", "sample_type": dtype, "window": window, "samples": BODY, "first_call_s": first,
                        "equal_positions": int((ref == out).sum().item()),
                        "max_abs_difference": float((ref.to(torch.float64) - out.to(torch.float64)).abs().max().item())}
                del ref
                if first < 5.0:
                    cases.append((trec, lambda ones=ones, window=window: _torch_form(x, ones, window), 1))
                else:
                    trec.update({"ms_median": first * 1e3, "ms_min": first * 1e3, "ms_max": first * 1e3, "reps": 1})
                    yield trec
            except Exception as e:                                   # (no float64 convolution in this build, or no memory for it)
                yield {"what": "torch", "sample_type": dtype, "window": window, "error": "%s: %s" % (type(e).__name__, str(e)[:200])}
            torch.cuda.empty_cache()
        cases.append((rec, level, a.calls))
        h_dev = torch.from_numpy(np.random.default_rng(window).standard_normal(window) / window).cuda()

        def filt(window=window, h_dev=h_dev):
            rc = L.sushi_hip_filter(x.data_ptr(), code, n, PAD, h_dev.data_ptr(), window, out.data_ptr(), BODY, st)
            assert rc == 0, rc

        cases.append(({"what": "filter", "sample_type": dtype, "n_taps": window, "samples": BODY}, filt, a.calls))
    for rec in _interleaved(cases, a.reps):
        if "bytes" in rec:
            rec["TB_per_s"] = rec["bytes"] / (rec["ms_median"] * 1e-3) / 1e12
        if rec["what"] == "level":
            rec["G_samples_per_s"] = BODY / (rec["ms_median"] * 1e-3) / 1e9
            rec["T_additions_per_s"] = BODY * rec["window"] / (rec["ms_median"] * 1e-3) / 1e12      # float32: one v_add_f64 each
        yield rec


def stream_cases(dtype, a):
    """WavStream.levelled end to end: the launch, fill_pads and the copy of the new row to the host for .data."""
    import torch
    from sushi_amd.wav import WavStream
    x = _row(dtype)
    w = WavStream.from_prepared(x.cpu().numpy().reshape(1, -1), 12000, BODY, PAD)
    w._dev_row = x                                               # as a loaded stream holds it: the row already in HBM
    for kw in ({}, {"window": 1023}):
        ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f = w.levelled(**kw)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            del f
        yield {"what": "WavStream.levelled", "label": a.label, "sample_type": dtype, "args": kw, "samples": BODY,
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
        raise SystemExit("level_rate.py measures on the GPU: none is visible")
    for dtype in ("uint8", "float32"):
        for rec in kernel_cases(dtype, a):
            print(json.dumps(rec), flush=True)
        if not a.no_baseline:
            for rec in stream_cases(dtype, a):
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
