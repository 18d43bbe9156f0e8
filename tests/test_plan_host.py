"""The plan of a batch on the CPU: sushi_amd/csrc/plan_core.hpp (host only) built with g++ into tests/host_plan_check.cpp, which
checks what a plan must be over a fixed table of cases; its --dump against the recorded plans (tests/golden/plan_cases.json);
and the library's own sushi_hip_batch_bytes against the same records -- the library and the check are the same code."""
import json
import os
import subprocess

import numpy as np
import pytest

from host_checks import build_check
from sushi_amd import _native

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("host_plan_check", tmp_path_factory.mktemp("plan_check"))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "plan_cases.json")) as f:
        return json.load(f)["cases"]


def test_every_planned_case_passes_its_checks(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_dump_equals_the_recorded_plans(check_exe, golden):
    out = subprocess.check_output([check_exe, "--dump"], text=True)
    got = [json.loads(line) for line in out.splitlines() if line.strip()]
    assert [c["name"] for c in got] == [c["name"] for c in golden]
    for g, want in zip(got, golden):
        assert sorted(g) == sorted(want), g["name"]
        for key in want:
            assert g[key] == want[key], (g["name"], key)


def test_library_sizes_every_case_as_recorded(check_exe, golden, tmp_path):
    """sushi_hip_batch_bytes, with SUSHI_HIP_LANES set to the case's override, returns the recorded total (0: refused)."""
    subprocess.check_call([check_exe, "--requests", str(tmp_path)])
    L = _native.lib()
    before = os.environ.pop("SUSHI_HIP_LANES", None)
    try:
        for case in golden:
            req = np.fromfile(os.path.join(tmp_path, case["name"] + ".req"), _native.REQUEST_DTYPE)
            assert len(req) == case["n"], case["name"]
            if case["lanes_override"]:
                os.environ["SUSHI_HIP_LANES"] = case["lanes_override"]
            else:
                os.environ.pop("SUSHI_HIP_LANES", None)
            got = L.sushi_hip_batch_bytes(req.ctypes.data, len(req), _native.PATH_FFT, -1, case["cap"])
            assert got == case["total"], (case["name"], got, case["total"])
            assert (got == 0) == (case["rc"] != 0), case["name"]
    finally:
        os.environ.pop("SUSHI_HIP_LANES", None)
        if before is not None:
            os.environ["SUSHI_HIP_LANES"] = before


def test_checks_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The same program with its own sanitizer runtime, run stand-alone (no environment, no preload): exit 0, nothing on stderr."""
    exe = build_check("host_plan_check", tmp_path, sanitize=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
