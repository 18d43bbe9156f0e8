"""The real-input forward transform of a pattern segment on the CPU (sushi_amd/csrc/fft_core.hpp "Forward transform of a REAL,
zero-padded pattern segment"; tspec_real_kernel): its index functions -- every bin stored exactly once, in the order the inverse
transform loads, every mirror the conjugate of its bin, rows 0 and 512 and bins 0, N/2 and 1024 r included --, the rule of its
switch (run_policy.hpp tspec_route), and its arithmetic in float32 against a float64 DFT of the padded segment
(tests/host_tspec_real_check.cpp, built with g++ and run as a program: no GPU, nothing loaded into Python)."""
import os
import subprocess

from fft_stage_ref import E_F
from host_checks import PLAIN, SANITIZED

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["length_1", "length_2", "length_3", "length_4095", "length_4096", "impulse_last", "constant", "alternating", "random",
         "random_offset"]


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "host_tspec_real_check.cpp"), "-o", exe])
    return exe


def _errors(exe):
    r = subprocess.run([exe, "errors"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    got = dict((line.split()[0], float(line.split()[1])) for line in r.stdout.splitlines())
    assert sorted(got) == sorted(CASES), got
    return got


def test_every_bin_is_stored_once_in_the_load_order_and_mirrors_are_conjugates(tmp_path):
    r = subprocess.run([_build(tmp_path, PLAIN, "host_tspec_real_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_float32_route_stays_within_the_forward_transforms_error_bound(tmp_path):
    """Relative 2-norm error of the 16384 bins against float64, per segment: within E_F, the bound of the
    complex route's 14 levels."""
    got = _errors(_build(tmp_path, PLAIN, "host_tspec_real_check"))
    print(got)
    for name in CASES:
        assert got[name] <= E_F, (name, got[name])


def test_the_check_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The same program with its own sanitizer runtime, run stand-alone: the index checks, then every segment again."""
    exe = _build(tmp_path, SANITIZED, "host_tspec_real_check_san")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    got = _errors(exe)
    for name in CASES:
        assert got[name] <= E_F, (name, got[name])
