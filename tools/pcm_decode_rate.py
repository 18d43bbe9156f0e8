"""Rate of sushi_hip_load_decode_format / sushi_hip_load_decode_mix_format.  GPU.

One 32 MB chunk (load.UPLOAD_CHUNK_BYTES: what one step of a load decodes) per sample format at 2 and at 6 channels, already in
HBM.  Per case, device time per call (HIP events around the library call alone; one warm-up, then the median / min / max of --reps
runs, all entries taken in turn within every repetition) of
  * sushi_hip_load_decode / sushi_hip_load_decode_mix on 16-BIT frames of the same count -- the existing entries, unchanged: the
    yardstick, never the code under test;
  * sushi_hip_load_decode_format (the mean) and sushi_hip_load_decode_mix_format with one output row and with eight.
The floor of an entry is (bytes in + 4 bytes out per frame and row) over 6.29 TB/s.  The new entries' results are compared with the
NumPy restatement on the first and last 64 K frames.

--load SECONDS also takes the wall time of one whole WavStream(path) load of a 48 kHz stereo programme of that length as a float32
file under formats='all', next to the same programme as a 16-bit file (each loaded twice; files in a temporary directory).

One JSON line per case.  Usage: python tools/pcm_decode_rate.py [--reps 20] [--load 1440]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 32 << 20
HBM_BYTES_PER_S = 6.29e12


def _time(fns, reps):
    """ms per call of every function in `fns`, taken in turn: {name: [reps values]}"""
    import torch
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


def _planted(pcm, sample_format):
    """Seeded bytes as they are for the integer formats; for the float ones the top byte is forced to 0x3F or 0xBF -- |v| in
    [0.5, 2) for 'f32', [2^-15, 2) for 'f64': samples around full scale (random bytes would be mostly huge or tiny values, and
    sums of huge ones end in NaNs, whose bit patterns no rule states)."""
    if sample_format not in ("f32", "f64"):
        return pcm
    width = 4 if sample_format == "f32" else 8
    v = pcm.view(-1, width)
    v[:, width - 1] = (v[:, width - 1] & 0x80) | 0x3F
    return pcm


def case(sample_format, channels, reps):
    import torch
    from sushi_amd import _native, downmix
    L = _native.lib()
    code, width = _native.PCM_FORMATS[sample_format], _native.PCM_WIDTHS[sample_format]
    fs = channels * width
    n = CHUNK_BYTES // fs
    g = torch.Generator(device="cuda").manual_seed(7)
    pcm = _planted(torch.randint(0, 256, (n * fs,), dtype=torch.uint8, device="cuda", generator=g), sample_format)
    pcm16 = torch.randint(0, 256, (n * channels * 2,), dtype=torch.uint8, device="cuda", generator=g)
    st = torch.cuda.current_stream().cuda_stream
    mono = torch.empty(n, dtype=torch.float32, device="cuda")
    rows = torch.empty((8, n), dtype=torch.float32, device="cuda")
    w = np.ascontiguousarray(np.random.default_rng(3).standard_normal((8, channels)).astype(np.float32))
    w[0] = 1.0 / channels

    def old_mean():
        assert L.sushi_hip_load_decode(pcm16.data_ptr(), n, channels, 2, mono.data_ptr(), st) == 0

    def old_mix(n_out):
        assert L.sushi_hip_load_decode_mix(pcm16.data_ptr(), n, channels, 2, w.ctypes.data, n_out, rows.data_ptr(), n, st) == 0

    def mean():
        assert L.sushi_hip_load_decode_format(pcm.data_ptr(), n, channels, code, mono.data_ptr(), st) == 0

    def mix(n_out):
        assert L.sushi_hip_load_decode_mix_format(pcm.data_ptr(), n, channels, code, w.ctypes.data, n_out, rows.data_ptr(), n, st) == 0

    ms = _time({"s16_mean": old_mean, "s16_mix1": lambda: old_mix(1), "s16_mix8": lambda: old_mix(8),
                "mean": mean, "mix1": lambda: mix(1), "mix8": lambda: mix(8)}, reps)
    # the results are the restatement's (the ends of the chunk: the whole of it takes NumPy a while)
    mean()
    mix(8)
    k = min(n, 1 << 16)
    for lo in (0, n - k):
        samples = downmix.samples_from_bytes(pcm[lo * fs:(lo + k) * fs].cpu().numpy().tobytes(), channels, sample_format)
        assert mono[lo:lo + k].cpu().numpy().tobytes() == downmix.mean_host(samples).tobytes()
        assert rows[:, lo:lo + k].cpu().numpy().tobytes() == downmix.mix_host(samples, w).tobytes()
    out = {"case": "%s_%dch" % (sample_format, channels), "sample_format": sample_format, "channels": channels, "frames": n,
           "pcm_bytes": n * fs, "reps": reps}
    for key, in_bytes, rows_written in (("s16_mean", n * channels * 2, 1), ("s16_mix1", n * channels * 2, 1),
                                        ("s16_mix8", n * channels * 2, 8), ("mean", n * fs, 1), ("mix1", n * fs, 1), ("mix8", n * fs, 8)):
        v = np.asarray(ms[key])
        nbytes = in_bytes + 4 * n * rows_written
        med = float(np.median(v))
        out[key] = {"ms_median": round(med, 4), "ms_min": round(float(v.min()), 4), "ms_max": round(float(v.max()), 4), "bytes": nbytes,
                    "gb_per_s": round(nbytes / (med * 1e-3) / 1e9, 1), "floor_ms": round(nbytes / HBM_BYTES_PER_S * 1e3, 4),
                    "over_floor": round(med / (nbytes / HBM_BYTES_PER_S * 1e3), 2)}
    for key in ("mean", "mix1", "mix8"):
        out[key + "_over_s16"] = round(out[key]["ms_median"] / out["s16_" + key]["ms_median"], 3)
    return out


def whole_load(seconds):
    """Wall time of WavStream(path) for one 48 kHz stereo programme as a 16-bit file (the default path) and as a float32 file
    (formats='all'): the file's read and upload are inside, as in any load."""
    import struct
    import torch
    from sushi_amd.wav import WavStream
    rate, channels = 48000, 2
    n = int(seconds * rate)
    rng = np.random.default_rng(5)
    out = {"case": "whole_load", "seconds": seconds, "rate": rate, "channels": channels, "frames": n}
    with tempfile.TemporaryDirectory(prefix="sushi_pcm_rate_") as d:
        paths = {"s16": os.path.join(d, "s16.wav"), "f32": os.path.join(d, "f32.wav")}
        with open(paths["s16"], "wb") as a, open(paths["f32"], "wb") as b:
            a.write(b"RIFF" + struct.pack("<L", 36 + n * 4) + b"WAVE" + b"fmt " +
                    struct.pack("<LHHLLHH", 16, 1, channels, rate, rate * 4, 4, 16) + b"data" + struct.pack("<L", n * 4))
            b.write(b"RIFF" + struct.pack("<L", 36 + n * 8) + b"WAVE" + b"fmt " +
                    struct.pack("<LHHLLHH", 16, 3, channels, rate, rate * 8, 8, 32) + b"data" + struct.pack("<L", n * 8))
            done = 0
            while done < n:                              # the same programme in both, ten seconds at a time
                m = min(10 * rate, n - done)
                x = (rng.standard_normal((m, channels)) * 4000).astype(np.int16)
                a.write(x.astype("<i2").tobytes())
                b.write((x.astype(np.float32) / np.float32(32768.0)).astype("<f4").tobytes())
                done += m
        out["file_bytes"] = {k: os.path.getsize(p) for k, p in paths.items()}
        streams = {}
        for run in (0, 1):
            for k, kw in (("s16", {}), ("f32", {"formats": "all"})):
                torch.cuda.synchronize()
                t = time.perf_counter()
                streams[k] = WavStream(paths[k], sample_type="float32", **kw)
                torch.cuda.synchronize()
                out.setdefault(k + "_load_s", []).append(round(time.perf_counter() - t, 3))
        out["same_bytes"] = streams["s16"].data.tobytes() == streams["f32"].data.tobytes()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--load", type=float, default=0.0, help="seconds of programme for the whole-load timing (0: none)")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pcm_decode_rate.py measures on the GPU: none is visible")
    from sushi_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    print(json.dumps({"library": os.path.relpath(_native.LIB_PATH, root)}), flush=True)
    for sample_format in _native.PCM_FORMATS:
        for channels in (2, 6):
            print(json.dumps(case(sample_format, channels, max(20, a.reps))), flush=True)
    if a.load > 0:
        print(json.dumps(whole_load(a.load)), flush=True)


if __name__ == "__main__":
    main()
