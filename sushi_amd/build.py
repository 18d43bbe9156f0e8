"""Build libsushi_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU).

The translation units (UNITS: one csrc/NAME.hip each, with the flags it needs and why) are compiled separately -- the direct MFMA
kernel alone takes ~3 min, the FFT unit ~35 s, the others seconds -- and linked.  What a unit depends on is read from its
#include "..." lines (unit_deps); the tables the FFT unit includes are written first (GENERATED); compile_command is the one place
the hipcc line exists.  Every unit sees csrc/sushi_geometry.hpp (through sushi_common.hpp): the sizes and records the host's plan
and the device code share.
"""
import functools
import math
import os
import re
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
HEADER = os.path.join(os.path.dirname(_HERE), "include", "sushi_hip.h")
LIB_DIR = os.path.join(_HERE, "lib")
OBJ_DIR = os.path.join(LIB_DIR, "obj")
LIB = os.path.join(LIB_DIR, "libsushi_hip.so")
TWIDDLE_INC = os.path.join(CSRC, "_gen_twiddle16384.inc")

# (name, flags): csrc/NAME.hip
# -ffp-contract=off for the three units cut from one (direct, exact, stream): their float64 epilogues and prefix sums restate
# cv2's operation order; a fused a*b-c*d would round differently from the reference (the hot loop is MFMA builtins, unaffected).
UNITS = [
    ("sushi_direct", ["-ffp-contract=off"]),    # direct path: the MFMA kernel and its launcher
    ("sushi_exact", ["-ffp-contract=off"]),     # FFT path's exact stages (refinement, tiles), unpack and fill kernels
    ("sushi_stream", ["-ffp-contract=off"]),    # stream preparation (prefix sums) and the stream C ABI (its parts: stream_core.hpp)
    # WavStream load pipeline (decode / downmix, weighted: downmix_core.hpp / decimate / pad / median clip / scale / quantise)
    ("sushi_load", ["-ffp-contract=off"]),      # NumPy's float32 operation order, no fused multiply-add
    # the decode for every sample format a WAV carries: 8-bit, 16- / 24- / 32-bit integer, float, double (pcm_core.hpp: the sample
    # rule, the mean and the mix on its values; a unit of its own: sushi_load's code does not change)
    ("sushi_pcm", ["-ffp-contract=off"]),       # the scale's product, and the mix's products and sums, round separately
    # whole score curves: i8 MFMA Toeplitz GEMM (uint8), canonical float64 chain (float32); the same tiles (curve_tiles.hpp)
    # evaluate the listed pairs of a threshold run and of a best-K run; what a curve call uploads and launches is host only
    # (curve_core.hpp)
    ("sushi_curve", ["-ffp-contract=off"]),     # the epilogue restates cv2's operation order (as sushi_direct.hip's)
    # a stream read at another speed: linear interpolation at a rational step (retime_core.hpp: the arithmetic, and the call's host
    # side; row_core.hpp: the step's cursor, and what every call on a row of samples checks and dispatches on)
    ("sushi_retime", ["-ffp-contract=off"]),    # NumPy's float64 operation order: product and sum round separately
    # a low-pass in front of the load pipeline's decimator: polyphase FIR at the file's rate (resample_core.hpp)
    ("sushi_resample", ["-ffp-contract=off"]),  # float64 taps: product and sum round separately, as NumPy's
    # a group of score rows on one shift axis, summed by weight and reduced to its first extremum (joint_core.hpp: the arithmetic,
    # and the call's host side)
    ("sushi_joint", ["-ffp-contract=off"]),     # NumPy's float64 operation order: product and sum round separately
    # score rows summed along sloped lines of shifts, one per candidate offset table row, reduced to the first extremum over all
    # (candidate, index) pairs (drift_core.hpp: the arithmetic, and the call's host side)
    ("sushi_drift", ["-ffp-contract=off"]),     # joint_accumulate unchanged: product and sum round separately
    # where the shift a sequence of score rows shares changes: a Viterbi pass with one price per change, one launch per row
    # (path_core.hpp: the arithmetic, and the call's host side)
    ("sushi_path", ["-ffp-contract=off"]),      # NumPy's float64 operation order: product and sum round separately
    # a shift that wanders: the same pass with moves of bounded reach between rows, a window minimum over an LDS-staged tile of the
    # row before; its margins, the same recurrence from the last row down over the kept forward rows and three first minima per
    # row; and the wide form of both, a reach up to 32767 where moves are free: per wide row a tile pass of prefix / suffix minima
    # (sushi_track_wide_tile.inc) and a step that combines a few of its records.  One unit, its step parts (the .inc files)
    # included once (track_core.hpp, track_margin_core.hpp, track_wide_core.hpp: the arithmetic, and the calls' host side;
    # path_device.hpp: what it shares with sushi_path)
    ("sushi_track", ["-ffp-contract=off"]),     # a move's price and its candidate round separately; M and C round once each
    # tracked events kept in order: the same four walks with a jump read per index from the prefix (margins: suffix) minimum of the
    # row before (after), and per row a scan of (minimum, first index) that writes it; the wide rows share sushi_track's tile pass
    # (track_order_core.hpp, track_order_margin_core.hpp: the combine rule, t and t', the jump sums, the calls' host side)
    ("sushi_track_order", ["-ffp-contract=off"]),       # track_core.hpp's candidates unchanged; the jump's sum rounds once
    # score rows clamped at a threshold: a fill and a scatter of a threshold run's hits, and the rule applied to rows that exist
    # (rows_core.hpp: the rule, the tiles, the search of a hit list, and the call's host side)
    ("sushi_rows", []),                         # comparisons and copies: no arithmetic to contract
    # a row's loudness contour: the mean absolute deviation about the sample type's centre over span blocks of hop samples, a tile
    # of blocks staged through LDS (envelope_core.hpp: the arithmetic, the tile, and the call's host side; row_core.hpp: a row's
    # sample with both clamps, its deviation, a row call's opening refusals)
    ("sushi_envelope", ["-ffp-contract=off"]),  # float64 sums in a stated order, each addition rounded once, as NumPy's
    # a row through a FIR filter of float64 taps about the sample type's centre: a tile's samples and the taps staged in LDS, a few
    # consecutive outputs a thread (filter_core.hpp: the arithmetic, the tile, and the call's host side; row_core.hpp as above)
    ("sushi_filter", ["-ffp-contract=off"]),    # float64: product and sum round separately, in ascending tap order, as NumPy's
    # a row divided by its local level, the mean absolute deviation over W samples around each: float32 sums |d| in float64 over
    # a tile staged in LDS, a few consecutive outputs a thread; uint8 takes the window sums from a prefix sum of the tile (wave
    # scans) (level_core.hpp: the arithmetic, both tiles, and the call's host side; row_core.hpp as above)
    ("sushi_level", ["-ffp-contract=off"]),     # float64: the sum's additions in ascending order, the quotient's operations one by one, as NumPy's
    # overlap-save FFT path; its parts, by stage, are csrc/sushi_fft_*.inc (included inside its anonymous namespace); the plan of
    # a batch (plan_core.hpp), what a handle holds about its requests and how it is staged (batch_core.hpp) and what a run decides
    # (run_policy.hpp) are host only
    # -fno-slp-vectorize: the SLP pass packs the complex MACs into v_pk_fma_f32 and pays for it in
    # register shuffles (v_mov / accvgpr traffic); plain v_fma_f32 already issues at the f32 peak rate.
    ("sushi_fft", ["-fno-slp-vectorize"]),
]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build libsushi_hip.so)")


def _write_if_changed(path, text):
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)
    return path


def write_twiddles(n=16384):
    """exp(-2*pi*i*k/n) as float32 literals (interleaved re, im), correctly rounded from float64."""
    import numpy as np
    k = np.arange(n, dtype=np.float64)
    ang = 2.0 * math.pi * k / n
    tab = np.empty(2 * n, np.float32)
    tab[0::2] = np.cos(ang)
    tab[1::2] = -np.sin(ang)
    text = "".join("%.9ef,%s" % (float(v), "\n" if i % 8 == 7 else " ") for i, v in enumerate(tab))
    return _write_if_changed(TWIDDLE_INC, text)


def _dft16_table(cols, index, parts):
    """A table of 16-point inverse DFT (DIR = +1) operands for the matrix pipe, as text: for each form (0: real parts of the
    result, 1: imaginary parts) a 64 x cols matrix, element (lane, j) the entry of row n, column k that index(lane, j) =
    (n, k, part) names -- part 0 multiplies the input's real parts, part 1 its imaginary parts; parts(vals) gives the float16
    arrays to emit for it, two halves to a 32-bit word."""
    import numpy as np
    words = []
    for form in (0, 1):
        vals = np.empty((64, cols), np.float64)
        for l in range(64):
            for j in range(cols):
                n, k, part = index(l, j)
                ang = 2.0 * math.pi * ((n * k) & 15) / 16.0
                wr, wi = math.cos(ang), math.sin(ang)
                vals[l, j] = (wr if part == 0 else -wi) if form == 0 else (wi if part == 0 else wr)
        words += [np.ascontiguousarray(p).view(np.uint32).reshape(-1) for p in parts(vals)]
    return "".join("0x%08xu,%s" % (int(v), "\n" if i % 8 == 7 else " ") for i, v in enumerate(np.concatenate(words)))


def _hilo(v):     # parts(vals): the high halves and what they leave; the high halves alone, times 2^-10
    hi = v.astype("float16")
    return [hi, (v - hi.astype("float64")).astype("float16")]


_scaled = lambda v: [(v * 2.0 ** -10).astype("float16")]
# index(lane, j): all 16 columns twice over (K = 32); the eight d1 of a low-band group (K = 16)
_full = lambda l, j: (l & 15, (8 * (l >> 4) + j) & 15, (8 * (l >> 4) + j) >> 4)
_low = lambda l, j: (l & 15, ((l >> 4) & 1) + (0, 2, 12, 14)[j], (l >> 4) >> 1)

DFT16_TABLES = [    # (file, cols, index, parts)
    # The B operands of ifft_kernel's first pass on the matrix pipe (fft_core.hpp dft16_operand): for each of the four products
    # (real parts of the result: high / low half of the matrix; imaginary parts: high / low) and each lane, eight halves as four
    # 32-bit words.  Inverse transform (DIR = +1).
    ("_gen_dft16_f16.inc", 8, _full, _hilo),
    # The B operands of bound_kernel's first pass (fft_core.hpp fft_wave_half_front): the DFT matrix's high halves only, times
    # 2^-10 -- [real parts of the result, imaginary parts][lane] x 8 halves as four 32-bit words.
    ("_gen_dft16_f16_bound.inc", 8, _full, _scaled),
    # The B operands of bound_low_kernel's first pass (fft_core.hpp fft_wave_half_front_low, dft16_low_operand): the rows of the
    # 16-point inverse DFT matrix for the eight d1 a low-band group holds, high halves times 2^-10 -- [real parts of the result,
    # imaginary parts][lane] x 4 halves as two 32-bit words (K = 16: v_mfma_f32_16x16x16_f16).
    ("_gen_dft16_f16_bound_low.inc", 4, _low, _scaled),
]


def _write_dft16(path, *table):
    return _write_if_changed(path, _dft16_table(*table))


# (path, writer) of every file the build writes into csrc before it compiles; a writer returns its path
GENERATED = [(TWIDDLE_INC, write_twiddles)] + [
    (os.path.join(CSRC, name), functools.partial(_write_dft16, os.path.join(CSRC, name), *table)) for name, *table in DFT16_TABLES]


def write_generated():
    return [writer() for _path, writer in GENERATED]


def unit_deps(name, csrc=CSRC):
    """Every file csrc/NAME.hip is compiled from: itself and the transitive closure of its #include "..." lines, each resolved
    relative to the including file (preprocessor conditions are ignored: too many dependencies only rebuild too much).  A file of
    GENERATED counts whether or not it is written yet; any other include that does not resolve is an error."""
    generated = {os.path.basename(p) for p, _writer in GENERATED}
    deps, todo = [], [os.path.join(csrc, name + ".hip")]
    while todo:
        path = todo.pop()
        if path in deps:
            continue
        deps.append(path)
        if os.path.basename(path) in generated:         # (a table: it includes nothing)
            continue
        with open(path) as f:
            for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', f.read(), re.M):
                dep = os.path.normpath(os.path.join(os.path.dirname(path), inc))
                if not os.path.exists(dep) and os.path.basename(dep) not in generated:
                    raise FileNotFoundError('%s includes "%s", which does not exist' % (path, inc))
                todo.append(dep)
    return deps


def compile_command(unit, out, mode, defines=(), extra=()):
    """The hipcc line of one unit.  mode: "obj" (an object file), "asm" (device assembly), "remarks" (an object file, with the
    compiler's kernel-resource-usage remarks on stderr)."""
    how = {"obj": ["-c"], "asm": ["--cuda-device-only", "-S"], "remarks": ["-Rpass-analysis=kernel-resource-usage", "-c"]}[mode]
    return [_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-Wall"] + list(defines) + \
        dict(UNITS)[unit] + list(extra) + how + [os.path.join(CSRC, unit + ".hip"), "-o", out]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    m = os.path.getmtime(target)
    return any(not os.path.exists(p) or os.path.getmtime(p) > m for p in deps)


def needs_build():
    return _stale(LIB, [p for p, _writer in GENERATED] + [p for name, _flags in UNITS for p in unit_deps(name)])


def build_native(force=False, verbose=False, defines=(), lib=None, obj_tag=""):
    """hipcc --offload-arch=gfx950 -O3 -c csrc/*.hip -> lib/obj/*.o -> lib/libsushi_hip.so
    `defines` / `lib` / `obj_tag`: a variant library beside the product one (tools/ A/B measurements)."""
    write_generated()
    lib = lib or LIB
    if not force and not defines and not needs_build():
        return lib
    os.makedirs(OBJ_DIR, exist_ok=True)
    objs, procs = [], []
    for name, _flags in UNITS:
        obj = os.path.join(OBJ_DIR, name + obj_tag + ".o")
        objs.append(obj)
        if force or _stale(obj, unit_deps(name)):
            cmd = compile_command(name, obj, "obj", defines)
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-fvisibility=hidden"] + objs + ["-o", lib]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return lib


if __name__ == "__main__":
    print(build_native(force=True, verbose=True))
