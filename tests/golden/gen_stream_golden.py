#!/usr/bin/env python3
"""Generate tests/golden/stream_stage.json: what tests/host_stream_check.cpp --dump prints -- for every stream case the size of its
buffer and where every SUSHI_HIP_VIEW_* lies in it, for every curve and retime case the launch facts and the size and FNV-1a digest
of the upload image (a few KB).

The fixture records where a stream's parts lie and the bytes a curve or retime call uploads (sushi_amd/csrc/stream_core.hpp,
curve_core.hpp, retime_core.hpp), so that the code can be rewritten against it: regenerate it only for a change that is MEANT to
change them, and say so.  Needs g++ only.
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "stream_stage.json")
sys.path.insert(0, os.path.dirname(HERE))
from host_checks import build_check  # noqa: E402


def main():
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.check_output([build_check("host_stream_check", tmp), "--dump"])
    with open(OUT, "wb") as f:
        f.write(out)
    print(OUT, len(out.splitlines()), "cases", len(out), "bytes")


if __name__ == "__main__":
    main()
