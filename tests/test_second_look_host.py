"""The index rules of the second look's loads and of the pair bound's stretches, on the CPU (sushi_amd/csrc/fft_core.hpp sl_in_band,
sl_sub, sl_entry; sushi_geometry.hpp slb_stretch; run_policy.hpp slb_route, second_look_route): tests/host_second_look_check.cpp,
built with g++ and run as a program, plain and under the address and undefined-behaviour sanitizers."""
import os
import subprocess

from host_checks import PLAIN, SANITIZED

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "host_second_look_check.cpp"), "-o", exe])
    return exe


def test_the_register_map_the_stretches_and_the_routes_pass_their_checks(tmp_path):
    r = subprocess.run([_build(tmp_path, PLAIN, "host_second_look_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_same_checks_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The program with its own sanitizer runtime, run stand-alone."""
    r = subprocess.run([_build(tmp_path, SANITIZED, "host_second_look_check_san")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
