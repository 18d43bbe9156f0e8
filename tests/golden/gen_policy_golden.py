#!/usr/bin/env python3
"""Generate tests/golden/policy_trace.json: what tests/host_policy_check.cpp --dump prints -- one JSON record per run and line of
four scripted sequences of runs (AUTO across a method switch, a suspension and two look-agains; the same under ALWAYS; a batch
that recovers; a reset in the middle), each with its inputs and every decision sushi_amd/csrc/run_policy.hpp took.

The fixture records what a run DECIDES, so that the code can be rewritten against it: regenerate it only for a change that is
MEANT to change a decision, and say so.  Needs g++ only.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "policy_trace.json")
sys.path.insert(0, os.path.dirname(HERE))
from host_checks import build_check  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.check_output([build_check("host_policy_check", tmp), "--dump"])
    with open(OUT, "wb") as f:
        f.write(out)
    print(OUT, len(out.splitlines()), "runs", len(out), "bytes")


if __name__ == "__main__":
    main()
