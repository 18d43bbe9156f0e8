#!/usr/bin/env python3
"""Registers / scratch / LDS / occupancy of every kernel of one translation unit, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks.  usage: tools/kernel_resources.py sushi_fft [extra hipcc flags ...]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sushi_amd import build  # noqa: E402

unit = sys.argv[1]
build.write_generated()
with tempfile.TemporaryDirectory() as tmp:
    cmd = build.compile_command(unit, os.path.join(tmp, unit + ".o"), "remarks", extra=sys.argv[2:])
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
rows, cur = [], None
for line in err.splitlines():
    m = re.search(r"remark: +(?:Function )?Name: (\S+)", line)
    if m:
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        cur = {"name": re.sub(r"\(anonymous namespace\)::|void ", "", name).split("(")[0]}
        rows.append(cur)
        continue
    m = re.search(r"remark: +([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
    if m and cur is not None:
        cur[m.group(1).strip()] = m.group(2)
    elif "error" in line:
        print(line)
print("%-44s %5s %5s %8s %7s %5s" % ("kernel", "VGPR", "SGPR", "scratch", "LDS", "occ"))
for r in rows:
    print("%-44s %5s %5s %8s %7s %5s" % (r["name"][:44], r.get("VGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize"),
                                          r.get("LDS Size"), r.get("Occupancy")))
