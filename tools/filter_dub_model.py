"""The dub model of DESIGN.md 3.28, on the CPU path (no GPU): a mono dub whose own speech sits in 300 - 3000 Hz over a shared bed.

Both streams share the bed (synth.make_dst_pcm(60, seed 0); the source's advanced by 1234 samples); each carries speech of its
own -- other noise through a 255-tap 300 - 3000 Hz band-pass -- at --level x the bed's rms.  The 24 events of the hum scenario
(tests/filter_cases.py) are searched over +-2 s with the CPU oracle, TM_SQDIFF_NORMED, on the streams as they are and after
filtered(low=300, high=3000, stop=True) on both.  One JSON line per sample type.  Usage: python tools/filter_dub_model.py [--level 8]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["SUSHI_HIP_LOAD"] = "host"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", type=float, default=8.0)
    a = ap.parse_args()
    import filter_cases as FC
    from oracle import oracle as O
    from sushi_amd import synth
    from sushi_amd.filter import band_taps
    from sushi_amd.wav import WavStream
    O.build()
    search = lambda row, pat: O.argmin_first(O.match_template_fft(row, pat, method=FC.SQ)[0])
    bed = synth.make_dst_pcm(FC.SECONDS, FC.RATE, seed=0).astype(np.float64)
    band = band_taps(FC.RATE, 300, 3000)

    def speech(seed):
        s = np.convolve(synth.make_dst_pcm(FC.SECONDS, FC.RATE, seed=seed).astype(np.float64), band, mode="same")
        return s * (a.level * np.sqrt(np.mean(bed ** 2) / np.mean(s ** 2)))

    dst_x = bed + speech(12)
    src_x = np.concatenate([bed[FC.OFFSET:], np.zeros(FC.OFFSET)]) + speech(13)
    evs = FC.events()
    for st in ("uint8", "float32"):
        dst = WavStream.from_samples(dst_x.astype(np.float32), FC.RATE, sample_type=st)
        src = WavStream.from_samples(src_x.astype(np.float32), FC.RATE, sample_type=st)
        raw = FC.found_shifts(dst, *FC.requests(src, evs), search)
        kw = {"low": 300, "high": 3000, "stop": True}
        f_dst, f_src = dst.filtered(**kw), src.filtered(**kw)
        got = FC.found_shifts(f_dst, *FC.requests(f_src, evs), search)
        print(json.dumps({"what": "dub model", "sample_type": st, "speech_level": a.level, "events": len(evs),
                          "unfiltered_at_true_shift": int((raw == FC.OFFSET).sum()),
                          "filtered_at_true_shift": int((got == FC.OFFSET).sum())}), flush=True)


if __name__ == "__main__":
    main()
