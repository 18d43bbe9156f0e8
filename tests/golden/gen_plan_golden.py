#!/usr/bin/env python3
"""Generate tests/golden/plan_cases.json: what tests/host_plan_check.cpp --dump prints for its table of cases -- for every case
the plan's totals, every field of every sub-batch of both cuts, FNV-1a digests of the sub-batches' schedules and items, and the
batch's device-memory layout (digests and sizes only: a few KB).

The fixture records what the plan of a batch IS (sushi_amd/csrc/plan_core.hpp), so that the code can be rewritten against it:
regenerate it only for a change that is MEANT to change a plan, and say so.  Needs g++ only.
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "plan_cases.json")
sys.path.insert(0, os.path.dirname(HERE))
from host_checks import build_check  # noqa: E402


def dump_cases(exe):
    """The records `exe --dump` prints, one per line."""
    out = subprocess.check_output([exe, "--dump"], text=True)
    return [json.loads(line) for line in out.splitlines() if line.strip()]


def main():
    with tempfile.TemporaryDirectory() as tmp:
        cases = dump_cases(build_check("host_plan_check", tmp))
    with open(OUT, "w") as f:
        f.write('{"generator":"tests/golden/gen_plan_golden.py","cases":[\n')
        f.write(",\n".join(json.dumps(c, separators=(",", ":")) for c in cases))
        f.write("\n]}\n")
    print(OUT, len(cases), "cases", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
