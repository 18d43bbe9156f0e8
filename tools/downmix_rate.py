"""Rate of sushi_hip_load_decode_mix.  GPU.

One 32 MB chunk (load.UPLOAD_CHUNK_BYTES: what one step of a load decodes) of 48 kHz 16-bit stereo and of 24-bit 6-channel PCM,
already in HBM.  Per input, device time per call (HIP events around the library call alone, median / min / max of --reps runs
after a warm-up, the three entries taken in turn within every repetition) of
  * sushi_hip_load_decode        -- the channel mean: the existing entry, unchanged, on the same buffer (the yardstick);
  * sushi_hip_load_decode_mix    -- one output row, and eight.
All three read the same bytes; they differ in the bytes written (4 B a frame and row).  The results of the new entry are compared
with mix_host on the first and last 64 K frames.

One JSON line per input.  Usage: python tools/downmix_rate.py [--reps 20]
(an A/B build of the library is measured by pointing SUSHI_HIP_LIB at it)
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 32 << 20


def _time(fns, reps):
    """ms per call of every function in `fns`, taken in turn: {name: [reps values]}"""
    import torch
    for _ in range(3):
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


def case(name, channels, width, reps):
    import torch
    from sushi_amd import _native, downmix
    L = _native.lib()
    fs = channels * width
    n = CHUNK_BYTES // fs
    g = torch.Generator(device="cuda").manual_seed(7)
    pcm = torch.randint(0, 256, (n * fs,), dtype=torch.uint8, device="cuda", generator=g)
    st = torch.cuda.current_stream().cuda_stream
    mono = torch.empty(n, dtype=torch.float32, device="cuda")
    rows = torch.empty((8, n), dtype=torch.float32, device="cuda")
    w = np.ascontiguousarray(np.random.default_rng(3).standard_normal((8, channels)).astype(np.float32))
    w[0] = 1.0 / channels

    def mean():
        rc = L.sushi_hip_load_decode(pcm.data_ptr(), n, channels, width, mono.data_ptr(), st)
        assert rc == 0, rc

    def mix(n_out):
        rc = L.sushi_hip_load_decode_mix(pcm.data_ptr(), n, channels, width, w.ctypes.data, n_out, rows.data_ptr(), n, st)
        assert rc == 0, rc

    ms = _time({"mean": mean, "mix1": lambda: mix(1), "mix8": lambda: mix(8)}, reps)
    # the rows are the restatement's (the ends of the chunk: the whole of it takes NumPy a while)
    mix(8)
    k = min(n, 1 << 16)
    for lo in (0, n - k):
        frames = downmix.frames_from_bytes(pcm[lo * fs:(lo + k) * fs].cpu().numpy().tobytes(), channels, width)
        assert rows[:, lo:lo + k].cpu().numpy().tobytes() == downmix.mix_host(frames, w).tobytes()
    out = {"case": name, "channels": channels, "sample_width": width, "frames": n, "pcm_bytes": n * fs, "reps": reps}
    for key, rows_written in (("mean", 1), ("mix1", 1), ("mix8", 8)):
        v = np.asarray(ms[key])
        nbytes = n * fs + 4 * n * rows_written
        out[key] = {"ms_median": round(float(np.median(v)), 4), "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4),
                    "bytes": nbytes, "gb_per_s": round(nbytes / (float(np.median(v)) * 1e-3) / 1e9, 1)}
    out["mix1_over_mean"] = round(out["mix1"]["ms_median"] / out["mean"]["ms_median"], 3)
    out["mean_spread"] = round((out["mean"]["ms_max"] - out["mean"]["ms_min"]) / out["mean"]["ms_median"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("downmix_rate.py measures on the GPU: none is visible")
    from sushi_amd import _native
    print(json.dumps({"library": _native.LIB_PATH}), flush=True)
    for name, channels, width in (("stereo16_48k", 2, 2), ("six24_48k", 6, 3)):
        print(json.dumps(case(name, channels, width, max(20, a.reps))), flush=True)


if __name__ == "__main__":
    main()
