"""What a run decides on the CPU: sushi_amd/csrc/run_policy.hpp (host only) built with g++ into tests/host_policy_check.cpp,
which states every rule as checks; and its --dump -- a model of a batch handle driven through scripted runs -- against the recorded
decisions (tests/golden/policy_trace.json)."""
import json
import os
import subprocess

import pytest

from host_checks import build_check

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("host_policy_check", tmp_path_factory.mktemp("policy_check"))


def test_every_rule_passes_its_checks(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_dump_equals_the_recorded_decisions(check_exe):
    with open(os.path.join(HERE, "golden", "policy_trace.json")) as f:
        want = f.read()
    got = subprocess.check_output([check_exe, "--dump"], text=True)
    assert got == want                                            # byte for byte
    runs = [json.loads(line) for line in got.splitlines()]
    assert {r["s"] for r in runs} == {"auto", "always", "recovers", "reset"}
    # (the records' fields by position: the header of tests/host_policy_check.cpp)
    suspended, whole_cut, voted, diag_suspended = (lambda r: r["form"][1]), (lambda r: r["form"][3]), (lambda r: r["subs"][0][3]), (lambda r: r["diag"][1])
    # what tests/test_pair_exclusion.py sees of the first scenario on the GPU: tried, suspended from run 1 on, looking again at 64 (and 128)
    auto = [r for r in runs if r["s"] == "auto"]
    assert len(auto) == 130 and [r["seq"] for r in auto if not diag_suspended(r)] == [0, 64, 128]
    assert [r["seq"] for r in auto if voted(r)] == [0, 64]
    always = [r for r in runs if r["s"] == "always"]
    assert len(always) == 130 and not any(suspended(r) or diag_suspended(r) for r in always)
    assert any(whole_cut(r) and not suspended(r) for r in runs if r["s"] == "recovers")


def test_checks_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The same program with its own sanitizer runtime, run stand-alone (no environment, no preload): exit 0, nothing on stderr."""
    exe = build_check("host_policy_check", tmp_path, sanitize=True)
    for args in ([], ["--dump"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr
