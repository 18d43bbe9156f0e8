"""The stand-alone CPU checks (tests/host_*_check.cpp, each with its own main): which g++ flags each is built with, and the one
function that builds them.  A check is run directly as a program, never loaded into Python."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))

PLAIN = ["-O2", "-std=c++17"]
# the sanitizer variant of a host-only header's check: the rules again, slowly, with every access and overflow watched
SANITIZED = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined"]
# these headers ARE the kernels' arithmetic and their units are built without contraction, so the check is too (bitwise
# comparisons with NumPy); always under the sanitizers, stopping at the first undefined operation
KERNEL_ARITHMETIC = PLAIN + ["-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]

FLAGS = {   # check: (flags, flags of its sanitizer variant or None)
    # float32 emulations of device code against float64 definitions, to a tolerance: speed matters, contraction does not
    "host_fft_check": (PLAIN, None),
    "host_mac_check": (PLAIN, None),
    "host_mfma_check": (PLAIN, None),
    # host-only integer logic (plan_core.hpp, batch_core.hpp, run_policy.hpp; stream_core.hpp, curve_core.hpp and the host part of
    # retime_core.hpp), compared with recorded output
    "host_plan_check": (PLAIN, SANITIZED),
    "host_batch_check": (PLAIN, SANITIZED),
    "host_policy_check": (PLAIN, SANITIZED),
    "host_stream_check": (PLAIN, SANITIZED),
    "host_downmix_check": (KERNEL_ARITHMETIC, None),
    "host_resample_check": (KERNEL_ARITHMETIC, None),
    "host_retime_check": (KERNEL_ARITHMETIC, None),
}


def build_check(name, out_dir, sanitize=False):
    """Compile tests/NAME.cpp into out_dir; the path of the executable."""
    flags = FLAGS[name][1 if sanitize else 0]
    exe = os.path.join(str(out_dir), name + ("_san" if sanitize else ""))
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, name + ".cpp"), "-o", exe])
    return exe
