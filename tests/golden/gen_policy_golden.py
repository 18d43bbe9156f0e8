#!/usr/bin/env python3
"""Generate tests/golden/policy_trace.json: what tests/host_policy_check.cpp --dump prints -- one JSON record per run and line of
four scripted sequences of runs (AUTO across a method switch, a suspension and two look-agains; the same under ALWAYS; a batch
that recovers; a reset in the middle), each with its inputs and every decision sushi_amd/csrc/run_policy.hpp took.

The fixture records what a run DECIDES, so that the code can be rewritten against it: regenerate it only for a change that is
MEANT to change a decision, and say so.  Needs g++ only.
"""
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "policy_trace.json")
SRC = os.path.join(os.path.dirname(HERE), "host_policy_check.cpp")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "host_policy_check")
        subprocess.check_call(["g++", "-O2", "-std=c++17", SRC, "-o", exe])
        out = subprocess.check_output([exe, "--dump"])
    with open(OUT, "wb") as f:
        f.write(out)
    print(OUT, len(out.splitlines()), "runs", len(out), "bytes")


if __name__ == "__main__":
    main()
