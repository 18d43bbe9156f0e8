#!/usr/bin/env python3
"""Generate tests/golden/batch_stage.json: what tests/host_batch_check.cpp --dump prints for the table of cases of
tests/batch_cases.hpp -- for every case the return code of stage_batch, the accounting, the size and FNV-1a digest of the upload
image, and device offset, size and digest of the two spans a run uploads for the one-sub-batch cut (digests and sizes only: a few KB).

The fixture records the bytes a batch handle uploads (sushi_amd/csrc/batch_core.hpp), so that the code can be rewritten against
it: regenerate it only for a change that is MEANT to change them, and say so.  Needs g++ only.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "batch_stage.json")
sys.path.insert(0, os.path.dirname(HERE))
from host_checks import build_check  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.check_output([build_check("host_batch_check", tmp), "--dump"])
    with open(OUT, "wb") as f:
        f.write(out)
    print(OUT, len(out.splitlines()), "cases", len(out), "bytes")


if __name__ == "__main__":
    main()
