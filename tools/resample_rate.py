"""Rate of sushi_hip_load_resample_fir.  GPU.

A 2-h mono float32 row already in HBM -- 345.6 M frames at 48 kHz, 317.52 M at 44.1 kHz -- decimated to 12 kHz into the padded row
the load pipeline builds (pad = 10 * frame rate on either side).  Per input, device time per call (HIP events around the library
call alone, median / min / max of --reps runs after a warm-up, the two entries taken in turn within every repetition) of
  * sushi_hip_load_resample      -- the nearest-neighbour decimation: the existing entry, unchanged, on the same row (the yardstick);
  * sushi_hip_load_resample_fir  -- the filter (its table uploaded once, outside the timing).
Beside each figure the two floors, from the chip constants of the micro-architecture guide: the bytes the call must move (the
input once, the row once) over the achievable HBM rate (6.29 TB/s measured), and its float64 operations -- 2 per tap and output,
not fused -- over the FP64 vector rate (half the FP32 vector peak of 157.3 TFLOPS, which counts a fused multiply-add as two:
39.3e12 separate float64 operations a second).  The filter's first and last 4096 body samples are compared with resample_host.

--load: also one whole WavStream(path) load of a 24-minute 48 kHz 16-bit stereo file (written to --tmp) under both settings, wall
time of the second of two loads each.

One JSON line per input.  Usage: python tools/resample_rate.py [--reps 20] [--load] [--tmp DIR]
(an A/B build of the library is measured by pointing SUSHI_HIP_LIB at it)
"""
import argparse
import json
import os
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 6.29e12
FP64_OPS_PER_S = 157.3e12 / 2 / 2
SECONDS = 2 * 3600


def _time(fns, reps):
    """ms per call of every function in `fns`, taken in turn: {name: [reps values]}"""
    import torch
    for _ in range(2):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


class _DeviceInput(object):
    """A device row as resample_host reads it: the frames at an index array, fetched when asked for."""
    ndim, dtype = 1, np.dtype(np.float32)

    def __init__(self, tensor):
        self.t, self.shape = tensor, (int(tensor.shape[0]),)

    def __getitem__(self, index):
        import torch
        return self.t[torch.from_numpy(np.ascontiguousarray(index, dtype=np.int64)).to(self.t.device)].cpu().numpy()


def case(fr, sr, reps):
    import torch
    from sushi_amd import _native, resample
    from sushi_amd.common import py2_round
    L = _native.lib()
    n_raw = SECONDS * fr
    g = torch.Generator(device="cuda").manual_seed(fr)
    raw = torch.randint(-32768, 32768, (n_raw,), dtype=torch.int32, device="cuda", generator=g).to(torch.float32)
    num, den, W, H = resample.fir_table(fr, sr)
    table = torch.from_numpy(np.array(H)).cuda()
    nl_full = int(py2_round(fr * (sr / float(fr))))
    n_body = SECONDS * nl_full
    pad = 10 * fr
    total = 2 * pad + n_body
    data = torch.empty(total, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    scale = 1.0 / (float(nl_full) / float(fr))

    def nearest():
        rc = L.sushi_hip_load_resample(raw.data_ptr(), n_raw, fr, nl_full, scale, SECONDS, 0, 0, 0.0, pad, total, data.data_ptr(), st)
        assert rc == 0, rc

    def fir():
        rc = L.sushi_hip_load_resample_fir(raw.data_ptr(), n_raw, num, den, table.data_ptr(), W, n_body, pad, total, data.data_ptr(), st)
        assert rc == 0, rc

    ms = _time({"nearest": nearest, "fir": fir}, reps)
    fir()
    x = _DeviceInput(raw)
    for first in (0, n_body - 4096):
        want = resample.resample_host(x, fr, sr, n_body, first=first, count=4096)
        assert data[pad + first:pad + first + 4096].cpu().numpy().tobytes() == want.tobytes(), first
    edge = data[torch.tensor([0, pad - 1, pad, total - pad - 1, total - pad, total - 1], device="cuda")].cpu().numpy()
    assert edge[0] == edge[1] == edge[2] and edge[3] == edge[4] == edge[5]
    out = {"case": "%d_to_%d" % (fr, sr), "frames": n_raw, "num": num, "den": den, "half_width": W, "n_body": n_body, "total": total,
           "reps": reps}
    moved = {"nearest": 4 * n_body + 4 * total, "fir": 4 * n_raw + 4 * total}      # nearest reads one frame per sample (a 32-byte sector each at 4:1: 8 x that from HBM)
    for key in ("nearest", "fir"):
        v = np.asarray(ms[key])
        out[key] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4),
                    "bytes": moved[key], "hbm_floor_ms": round(moved[key] / HBM_BYTES_PER_S * 1e3, 4)}
    ops = n_body * 2 * W * 2
    out["fir"]["fp64_ops"] = ops
    out["fir"]["fp64_floor_ms"] = round(ops / FP64_OPS_PER_S * 1e3, 4)
    out["fir"]["over_larger_floor"] = round(out["fir"]["ms_median"] / max(out["fir"]["fp64_floor_ms"], out["fir"]["hbm_floor_ms"]), 2)
    out["fir_over_nearest"] = round(out["fir"]["ms_median"] / out["nearest"]["ms_median"], 2)
    return out


def whole_load(tmp):
    import torch
    from sushi_amd.wav import WavStream
    rate, channels, seconds = 48000, 2, 24 * 60
    path = os.path.join(tmp, "resample_rate_long.wav")
    second = (np.random.default_rng(3).standard_normal((rate, channels)) * 3000).astype('<i2').tobytes()
    n_bytes = len(second) * seconds
    with open(path, "wb") as f:
        f.write(b'RIFF' + struct.pack('<L', 36 + n_bytes) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<LHHLLHH', 16, 1, channels, rate, rate * channels * 2, channels * 2, 16))
        f.write(b'data' + struct.pack('<L', n_bytes))
        for _ in range(seconds):
            f.write(second)
    out = {"case": "wavstream_24min_48k_stereo16", "file_bytes": n_bytes + 44}
    try:
        for mode in ("nearest", "fir", "nearest", "fir"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s = WavStream(path, sample_rate=12000, sample_type='uint8', resample=mode)
            torch.cuda.synchronize()
            out[mode + "_s"] = round(time.perf_counter() - t0, 4)           # (the second load of each mode stays)
            assert s.data.shape == (1, 20 * rate + seconds * 12000)
    finally:
        os.remove(path)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--load", action="store_true")
    ap.add_argument("--tmp", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resample_rate.py measures on the GPU: none is visible")
    from sushi_amd import _native
    print(json.dumps({"library": _native.LIB_PATH}), flush=True)
    for fr in (48000, 44100):
        print(json.dumps(case(fr, 12000, max(20, a.reps))), flush=True)
        torch.cuda.empty_cache()
    if a.load:
        import tempfile
        print(json.dumps(whole_load(a.tmp or tempfile.gettempdir())), flush=True)


if __name__ == "__main__":
    main()
