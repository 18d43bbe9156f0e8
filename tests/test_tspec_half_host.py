"""The half rows the real route stores of a pattern segment's spectrum, on the CPU (sushi_amd/csrc/fft_core.hpp "HALF ROWS"):
whole rows that are conjugate-symmetric word for word by the kernel's own rule -- zero imaginary halves under real halves of
either sign, an all-zero row, random words, rows 0 and 512 --, their half rows taken the way tspec_real_kernel stores them (every
stored entry and both of row 1024's written exactly once), and every word of all 4096 entries given back by the one function every
reader goes through; the sources of every mirrored run (one stored run reversed, two for the eight runs beside row 0); the mirror
entries of mac_rows_kernel's paired first pass; the flag's rule per route (run_policy.hpp tspec_half_rows) and what it sizes
(plan_core.hpp ws_layout).  tests/host_tspec_half_check.cpp, built with g++ and run as a program: no GPU, nothing loaded into Python."""
import os
import subprocess

from host_checks import PLAIN, SANITIZED

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "host_tspec_half_check.cpp"), "-o", exe])
    return exe


def test_half_rows_give_back_every_word_of_the_whole_row(tmp_path):
    r = subprocess.run([_build(tmp_path, PLAIN, "host_tspec_half_check")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr


def test_the_check_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The same program with its own sanitizer runtime, run stand-alone."""
    r = subprocess.run([_build(tmp_path, SANITIZED, "host_tspec_half_check_san")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
