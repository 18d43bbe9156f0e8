"""How the band-split form's pilots get their whole rows (sushi_amd/csrc/run_policy.hpp pilot_rows_route: SUSHI_HIP_PILOT_ROWS), on the
CPU: tests/host_pilot_rows_check.cpp built with g++ and run as a program."""
import os
import subprocess

from host_checks import PLAIN, SANITIZED

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "host_pilot_rows_check.cpp"), "-o", exe])
    return exe


def test_the_route_rule_passes_its_checks(tmp_path):
    r = subprocess.run([_build(tmp_path, PLAIN, "host_pilot_rows_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_check_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The same program with its own sanitizer runtime, run stand-alone: exit 0, nothing on stderr."""
    r = subprocess.run([_build(tmp_path, SANITIZED, "host_pilot_rows_check_san")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
