#!/usr/bin/env python3
"""Generate tests/golden/load_paths.json: what every constructor of WavStream makes of the inputs of tests/load_paths_cases.py,
on the NumPy load path (SUSHI_HIP_LOAD=host).

It pins the loader to itself: run it at the commit whose behaviour is to be kept, commit the result, and tests/test_load_paths.py
holds every later commit -- and the GPU path -- to those bytes.  Needs nothing but the repository.
"""
import json
import os
import sys
import tempfile

os.environ["SUSHI_HIP_LOAD"] = "host"

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "load_paths.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import load_paths_cases as cases  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for name in cases.INPUTS:
            path, top, rate = cases.write_input(d, name)
            for sample_type in cases.SAMPLE_TYPES:
                for resample in cases.RESAMPLE_MODES:
                    for how in cases.CONSTRUCTORS:
                        got, _ = cases.outcome(how, path, top, rate, sample_type, resample)
                        out[cases.key(name, sample_type, resample, how)] = got
                        print(cases.key(name, sample_type, resample, how), got.get("error") or [s["sha256"][:12] for s in got["streams"]])
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/gen_load_paths_golden.py", "cases": out}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "cases")


if __name__ == "__main__":
    main()
