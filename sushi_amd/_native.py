"""ctypes binding of libsushi_hip.so (C ABI: include/sushi_hip.h).

There is no CPU fallback: if the library is missing or a call fails, the product path raises.
"""
import ctypes
import os
import re

import numpy as np

from .common import SushiError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SUSHI_HIP_LIB") or os.path.join(_HERE, "lib", "libsushi_hip.so")   # env: dev A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sushi_hip.h")

# dtype codes / paths (include/sushi_hip.h)
U8, F32 = 0, 1
PATH_FFT, PATH_DIRECT = 0, 1
METHOD_SQDIFF_NORMED, METHOD_CCOEFF_NORMED = 0, 1       # cv2.TM_SQDIFF_NORMED + argmin (wav.py:185-186) | cv2.TM_CCOEFF_NORMED + argmax
MIX_MAX_CHANNELS, MIX_MAX_OUTPUTS = 32, 8    # SUSHI_HIP_MIX_MAX_*: channels and output rows of sushi_hip_load_decode_mix
# SUSHI_HIP_PCM_*: the sample formats of sushi_hip_load_decode_format / _decode_mix_format, and their container bytes
PCM_FORMATS = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 5, "f64": 6}
PCM_WIDTHS = {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 4, "f64": 8}
BEST_MAX_K = 32            # SUSHI_HIP_BEST_MAX_K: picks per request of a best-K run (sushi_hip_batch_run_best)
TRACK_MAX_REACH, TRACK_JUMP = 1024, -32768   # SUSHI_HIP_TRACK_*: the widest move between two events, and the move word of a jump
TRACK_WIDE_MAX_REACH = 32767     # SUSHI_HIP_TRACK_WIDE_MAX_REACH: the widest move of the wide pass (a free move: step_cost 0)
TRACK_BACK_ANY = -1        # SUSHI_HIP_TRACK_BACK_ANY: a back that leaves a jump free to come from anywhere
METHODS = {"sqdiff_normed": METHOD_SQDIFF_NORMED, "ccoeff_normed": METHOD_CCOEFF_NORMED}
VIEW_XC, VIEW_S1, VIEW_S2, VIEW_UREL, VIEW_BASE, VIEW_SPECTRA, VIEW_USREL, VIEW_BASE1, VIEW_COARSE, VIEW_SPECTRA_LOW, \
    VIEW_ZNORM_REST = range(11)

ABI_VERSION = 13
ENOSPACE = -4              # SUSHI_HIP_ENOSPACE: buffer or workspace too small
NSTAGES = 6
STAGE_NAMES = ("tspec", "mac", "ifft", "refine", "finish", "bound")
STAGE_KERNELS = {"tspec": "tspec_real_kernel|tspec_kernel", "mac": "mac_kernel", "ifft": "mac_list_kernel+mac_rows_kernel+ifft_kernel", "refine": "refine_kernel",
                 "finish": "collect_kernel+exact_tiles_kernel+unpack_keys_kernel", "bound": "bound_low_kernel|bound_kernel"}
EXCLUSION = {"auto": 0, "always": 1, "never": 2, "band": 3, "whole": 4}        # SUSHI_HIP_EXCLUDE_*
WS_TSPEC, WS_Y, WS_TSPEC_LOW, WS_Y_LOW, WS_TNORM_REST, WS_TSPEC_HALF = range(6)                           # SUSHI_HIP_WS_*
WS_SLIST, WS_SLIST2, WS_SCOUNT, WS_MARKS, WS_PAIR_LB = range(6, 11)              # ... what the pair exclusion left, for its tests
BOUND_MODEL = {"worst_case": 0, "statistical": 1}                              # SUSHI_HIP_BOUND_*
# every kernel a stage's HIP-event span covers (profiles/pmc_traffic.json is keyed by kernel)
STAGE_KERNEL_SETS = {"tspec": ("tspec_real_kernel", "tspec_kernel"), "mac": ("mac_kernel", "mac_long_kernel"),
                     "ifft": ("ifft_kernel", "ifft_list_kernel", "pilot_kernel", "survivor_kernel", "mac_list_kernel", "mac_rows_kernel",
                              "bound_low_exact_kernel", "slb_list_kernel", "survivor2_kernel"),
                     "refine": ("refine_kernel",),
                     "finish": ("collect_kernel", "exact_tiles_kernel"), "bound": ("bound_kernel", "bound_low_kernel", "slb_kernel")}

# struct SushiHipRequest, 24 bytes
REQUEST_DTYPE = np.dtype([("tmpl_off", "<i8"), ("win_start", "<i8"), ("tmpl_len", "<i4"), ("n_pos", "<i4")], align=True)
assert REQUEST_DTYPE.itemsize == 24
# struct SushiHipHit, 8 bytes: one position of a threshold run (sushi_hip_batch_run_threshold) and its float32 score
HIT_DTYPE = np.dtype([("index", "<i4"), ("score", "<f4")], align=True)
assert HIT_DTYPE.itemsize == 8
# struct SushiHipRetimeSegment, 32 bytes: one segment of a retime call (sushi_hip_retime)
RETIME_SEGMENT_DTYPE = np.dtype([("in_start", "<i8"), ("out_off", "<i8"), ("out_len", "<i8"), ("num", "<i4"), ("den", "<i4")], align=True)
assert RETIME_SEGMENT_DTYPE.itemsize == 32
# struct SushiHipJointRow / SushiHipJointGroup, 16 bytes each: the tables of a joint call (sushi_hip_joint_reduce)
JOINT_ROW_DTYPE = np.dtype([("curve_off", "<i8"), ("weight", "<f8")], align=True)
assert JOINT_ROW_DTYPE.itemsize == 16
JOINT_GROUP_DTYPE = np.dtype([("first_row", "<i4"), ("n_rows", "<i4"), ("n_shift", "<i4"), ("reserved", "<i4")], align=True)
assert JOINT_GROUP_DTYPE.itemsize == 16
# struct SushiHipRowsRow, 24 bytes: where a row lies in the buffers of a rows call (sushi_hip_rows_from_hits / sushi_hip_rows_clamp)
ROWS_ROW_DTYPE = np.dtype([("out_off", "<i8"), ("in_off", "<i8"), ("n_pos", "<i4"), ("reserved", "<i4")], align=True)
assert ROWS_ROW_DTYPE.itemsize == 24
ROWS_OVERFLOW, ROWS_BAD_HITS = 1, 2          # SUSHI_HIP_ROWS_*: the flag bits of sushi_hip_rows_from_hits


class BatchInfo(ctypes.Structure):
    _fields_ = [("n_search", ctypes.c_int32), ("path", ctypes.c_int32), ("variant", ctypes.c_int32),
                ("sub_batches", ctypes.c_int32), ("direct_tiles", ctypes.c_int64), ("fft_pairs", ctypes.c_int64),
                ("fft_segments", ctypes.c_int64), ("workspace_bytes", ctypes.c_uint64), ("mem_bytes", ctypes.c_uint64),
                ("flops", ctypes.c_double), ("algorithmic_bytes", ctypes.c_double), ("lanes", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class BatchDiag(ctypes.Structure):
    _fields_ = [("flagged", ctypes.c_int32), ("all_positions", ctypes.c_int32), ("tiles_dense", ctypes.c_int64),
                ("tiles_sparse", ctypes.c_int64), ("candidates", ctypes.c_int64), ("max_bound_ratio", ctypes.c_float),
                ("max_bound_ratio_noncandidate", ctypes.c_float), ("audited", ctypes.c_int64),
                ("pairs_transformed", ctypes.c_int64), ("excluded_audited", ctypes.c_int64),
                ("max_slb_ratio_excluded", ctypes.c_float), ("slb_violations", ctypes.c_int32), ("band", ctypes.c_int32),
                ("suspended", ctypes.c_int32), ("band_votes", ctypes.c_int32 * 2), ("second_look_audited", ctypes.c_int64)]


_lib = None


class NativeError(SushiError):
    pass


def declared_symbols():
    """Every function include/sushi_hip.h declares (used by the CPU-side export test)."""
    with open(HEADER_PATH) as f:
        text = f.read()
    return sorted(set(re.findall(r"SUSHI_HIP_API\s+[\w\s\*]+?\b(sushi_hip_\w+)\s*\(", text)))


def lib():
    """Load (once) and type the library.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError("libsushi_hip.so is not built (%s); run `python -m sushi_amd.build` -- "
                          "there is no CPU fallback for the matching path" % LIB_PATH)
    # PyTorch-ROCm ships its own HIP runtime (same SONAME as /opt/rocm's).  Whichever is mapped first serves the
    # whole process, and torch cannot see the GPU through the other one: torch first, then our library.
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    vp, i64, ci, dbl, sz = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_size_t
    i32, u32, cf = ctypes.c_int32, ctypes.c_uint32, ctypes.c_float
    pvp = ctypes.POINTER(vp)
    L.sushi_hip_abi_version.restype = ci
    L.sushi_hip_strerror.restype = ctypes.c_char_p
    L.sushi_hip_strerror.argtypes = [ci]
    L.sushi_hip_device_ok.restype = ci
    L.sushi_hip_device_prepare.restype = ci
    L.sushi_hip_fft_size.restype = ci
    L.sushi_hip_fft_block.restype = ci
    L.sushi_hip_fft_slot_of_bin.restype = ci
    L.sushi_hip_fft_slot_of_bin.argtypes = [ci]
    L.sushi_hip_fft_low_slot_of_bin.restype = ci
    L.sushi_hip_fft_low_slot_of_bin.argtypes = [ci]
    L.sushi_hip_centre.restype = dbl
    L.sushi_hip_centre.argtypes = [ci]
    L.sushi_hip_stream_bytes.restype = sz
    L.sushi_hip_stream_bytes.argtypes = [i64, ci, ci]
    L.sushi_hip_stream_spectra_bytes.restype = sz
    L.sushi_hip_stream_spectra_bytes.argtypes = [i64]
    L.sushi_hip_stream_create.restype = ci
    L.sushi_hip_stream_create.argtypes = [vp, ci, i64, ci, vp, sz, vp, pvp]
    L.sushi_hip_stream_add_spectra.restype = ci
    L.sushi_hip_stream_add_spectra.argtypes = [vp, vp, sz, vp]
    L.sushi_hip_stream_view.restype = ci
    L.sushi_hip_stream_view.argtypes = [vp, ci, pvp, ctypes.POINTER(sz)]
    L.sushi_hip_stream_destroy.restype = None
    L.sushi_hip_stream_destroy.argtypes = [vp]
    L.sushi_hip_batch_bytes.restype = sz
    L.sushi_hip_batch_bytes.argtypes = [vp, ci, ci, ci, sz]
    L.sushi_hip_batch_create.restype = ci
    L.sushi_hip_batch_create.argtypes = [vp, vp, vp, ci, ci, ci, sz, vp, sz, vp, pvp]
    L.sushi_hip_batch_reset.restype = ci
    L.sushi_hip_batch_reset.argtypes = [vp, vp, ci, vp]
    L.sushi_hip_batch_info.restype = ci
    L.sushi_hip_batch_info.argtypes = [vp, ctypes.POINTER(BatchInfo)]
    L.sushi_hip_batch_set_method.restype = ci
    L.sushi_hip_batch_set_method.argtypes = [vp, ci]
    L.sushi_hip_batch_run.restype = ci
    L.sushi_hip_batch_run.argtypes = [vp, dbl, vp, vp, vp]
    L.sushi_hip_batch_run_threshold.restype = ci
    L.sushi_hip_batch_run_threshold.argtypes = [vp, dbl, i32, vp, vp, vp]
    L.sushi_hip_batch_run_best.restype = ci
    L.sushi_hip_batch_run_best.argtypes = [vp, i32, i32, ctypes.POINTER(dbl), vp, vp, vp]
    L.sushi_hip_batch_diagnostics.restype = ci
    L.sushi_hip_batch_diagnostics.argtypes = [vp, ctypes.POINTER(BatchDiag), vp, vp]
    L.sushi_hip_batch_set_packed_output.restype = ci
    L.sushi_hip_batch_set_packed_output.argtypes = [vp, vp]
    L.sushi_hip_batch_set_early_output.restype = ci
    L.sushi_hip_batch_set_early_output.argtypes = [vp, vp]
    L.sushi_hip_batch_set_exclusion.restype = ci
    L.sushi_hip_batch_set_exclusion.argtypes = [vp, ci]
    L.sushi_hip_batch_set_bound_model.restype = ci
    L.sushi_hip_batch_set_bound_model.argtypes = [vp, ci]
    L.sushi_hip_batch_pair_bounds.restype = ci
    L.sushi_hip_batch_pair_bounds.argtypes = [vp, vp, vp, ctypes.POINTER(i64)]
    if hasattr(L, "sushi_hip_batch_bounds_again"):          # (SUSHI_HIP_LIB may name a library built before the tests' seam)
        L.sushi_hip_batch_bounds_again.restype = ci
        L.sushi_hip_batch_bounds_again.argtypes = [vp, ci, ci, vp, vp, ctypes.POINTER(i64)]
    L.sushi_hip_batch_workspace_view.restype = ci
    L.sushi_hip_batch_workspace_view.argtypes = [vp, ci, pvp, ctypes.POINTER(sz)]
    L.sushi_hip_batch_destroy.restype = None
    L.sushi_hip_batch_destroy.argtypes = [vp]
    L.sushi_hip_fft_layout.restype = ci
    L.sushi_hip_fft_layout.argtypes = [i64, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    L.sushi_hip_curve_bytes.restype = sz
    L.sushi_hip_curve_bytes.argtypes = [vp, ci]
    L.sushi_hip_match_curves.restype = ci
    L.sushi_hip_match_curves.argtypes = [vp, vp, vp, ci, ci, vp, sz, vp, vp]
    L.sushi_hip_retime_bytes.restype = sz
    L.sushi_hip_retime_bytes.argtypes = [ci]
    L.sushi_hip_retime.restype = ci
    L.sushi_hip_retime.argtypes = [vp, ci, i64, vp, ci, vp, i64, vp, sz, vp]
    L.sushi_hip_envelope.restype = ci
    L.sushi_hip_envelope.argtypes = [vp, ci, i64, i64, i32, i32, vp, i64, vp]
    L.sushi_hip_filter.restype = ci
    L.sushi_hip_filter.argtypes = [vp, ci, i64, i64, vp, i32, vp, i64, vp]
    L.sushi_hip_level.restype = ci
    L.sushi_hip_level.argtypes = [vp, ci, i64, i64, i32, dbl, dbl, vp, i64, vp]
    L.sushi_hip_joint_bytes.restype = sz
    L.sushi_hip_joint_bytes.argtypes = [ci, ci]
    L.sushi_hip_joint_reduce.restype = ci
    L.sushi_hip_joint_reduce.argtypes = [vp, i64, vp, ci, vp, ci, ci, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.sushi_hip_drift_bytes.restype = sz
    L.sushi_hip_drift_bytes.argtypes = [ci, ci]
    L.sushi_hip_drift_reduce.restype = ci
    L.sushi_hip_drift_reduce.argtypes = [vp, i64, vp, ci, i32, vp, ci, ci, vp, sz, vp, vp, vp, vp, vp, vp, vp]
    L.sushi_hip_path_bytes.restype = sz
    L.sushi_hip_path_bytes.argtypes = [ci, i32]
    L.sushi_hip_path_stay_words.restype = i64
    L.sushi_hip_path_stay_words.argtypes = [i32]
    L.sushi_hip_path_forward.restype = ci
    L.sushi_hip_path_forward.argtypes = [vp, i64, vp, ci, i32, ci, dbl, ci, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sushi_hip_path_backtrack.restype = ci
    L.sushi_hip_path_backtrack.argtypes = [vp, vp, ci, i32, vp, vp]
    L.sushi_hip_track_bytes.restype = sz
    L.sushi_hip_track_bytes.argtypes = [ci, i32]
    L.sushi_hip_track_forward.restype = ci
    L.sushi_hip_track_forward.argtypes = [vp, i64, vp, vp, ci, i32, ci, dbl, dbl, ci, ci, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.sushi_hip_track_backtrack.restype = ci
    L.sushi_hip_track_backtrack.argtypes = [vp, vp, ci, i32, vp, vp]
    L.sushi_hip_track_forward_keep.restype = ci
    L.sushi_hip_track_forward_keep.argtypes = L.sushi_hip_track_forward.argtypes
    L.sushi_hip_track_margins_bytes.restype = sz
    L.sushi_hip_track_margins_bytes.argtypes = [ci, i32]
    L.sushi_hip_track_margins.restype = ci
    L.sushi_hip_track_margins.argtypes = [vp, i64, vp, vp, vp, ci, i32, ci, dbl, dbl, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                          sz, vp]
    L.sushi_hip_track_wide_bytes.restype = sz
    L.sushi_hip_track_wide_bytes.argtypes = [ci, i32]
    L.sushi_hip_track_margins_wide_bytes.restype = sz
    L.sushi_hip_track_margins_wide_bytes.argtypes = [ci, i32]
    L.sushi_hip_track_forward_wide.restype = ci
    L.sushi_hip_track_forward_wide.argtypes = L.sushi_hip_track_forward.argtypes
    L.sushi_hip_track_forward_wide_keep.restype = ci
    L.sushi_hip_track_forward_wide_keep.argtypes = L.sushi_hip_track_forward.argtypes
    L.sushi_hip_track_margins_wide.restype = ci
    L.sushi_hip_track_margins_wide.argtypes = L.sushi_hip_track_margins.argtypes
    L.sushi_hip_track_order_bytes.restype = sz
    L.sushi_hip_track_order_bytes.argtypes = [ci, i32]
    L.sushi_hip_track_forward_ordered.restype = ci
    L.sushi_hip_track_forward_ordered.argtypes = [vp, i64, vp, vp, vp, ci, i32, ci, vp, dbl, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                  vp, sz, vp]
    L.sushi_hip_track_backtrack_ordered.restype = ci
    L.sushi_hip_track_backtrack_ordered.argtypes = [vp, vp, vp, vp, ci, i32, vp, vp]
    L.sushi_hip_track_forward_ordered_keep.restype = ci
    L.sushi_hip_track_forward_ordered_keep.argtypes = L.sushi_hip_track_forward_ordered.argtypes
    L.sushi_hip_track_order_margins_bytes.restype = sz
    L.sushi_hip_track_order_margins_bytes.argtypes = [ci, i32]
    L.sushi_hip_track_order_margins.restype = ci
    L.sushi_hip_track_order_margins.argtypes = [vp, i64, vp, vp, vp, vp, ci, i32, ci, vp, dbl, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                                vp, vp, vp, sz, vp]
    L.sushi_hip_track_order_wide_bytes.restype = sz
    L.sushi_hip_track_order_wide_bytes.argtypes = [ci, i32]
    L.sushi_hip_track_order_margins_wide_bytes.restype = sz
    L.sushi_hip_track_order_margins_wide_bytes.argtypes = [ci, i32]
    L.sushi_hip_track_forward_ordered_wide.restype = ci
    L.sushi_hip_track_forward_ordered_wide.argtypes = L.sushi_hip_track_forward_ordered.argtypes
    L.sushi_hip_track_forward_ordered_wide_keep.restype = ci
    L.sushi_hip_track_forward_ordered_wide_keep.argtypes = L.sushi_hip_track_forward_ordered.argtypes
    L.sushi_hip_track_order_margins_wide.restype = ci
    L.sushi_hip_track_order_margins_wide.argtypes = L.sushi_hip_track_order_margins.argtypes
    L.sushi_hip_rows_tile.restype = ci
    L.sushi_hip_rows_bytes.restype = sz
    L.sushi_hip_rows_bytes.argtypes = [ci]
    L.sushi_hip_rows_from_hits.restype = ci
    L.sushi_hip_rows_from_hits.argtypes = [vp, vp, ci, i32, vp, cf, vp, i64, vp, vp, sz, vp]
    L.sushi_hip_rows_clamp.restype = ci
    L.sushi_hip_rows_clamp.argtypes = [vp, i64, vp, i64, vp, ci, ci, cf, vp, sz, vp]
    L.sushi_hip_load_decode.restype = ci
    L.sushi_hip_load_decode.argtypes = [vp, i64, i32, i32, vp, vp]
    L.sushi_hip_load_decode_mix.restype = ci
    L.sushi_hip_load_decode_mix.argtypes = [vp, i64, i32, i32, vp, i32, vp, i64, vp]
    L.sushi_hip_load_decode_format.restype = ci
    L.sushi_hip_load_decode_format.argtypes = [vp, i64, i32, i32, vp, vp]
    L.sushi_hip_load_decode_mix_format.restype = ci
    L.sushi_hip_load_decode_mix_format.argtypes = [vp, i64, i32, i32, vp, i32, vp, i64, vp]
    L.sushi_hip_load_resample.restype = ci
    L.sushi_hip_load_resample.argtypes = [vp, i64, i32, i32, dbl, i64, i32, i32, dbl, i64, i64, vp, vp]
    L.sushi_hip_load_resample_fir.restype = ci
    L.sushi_hip_load_resample_fir.argtypes = [vp, i64, i32, i32, vp, i32, i64, i64, i64, vp, vp]
    L.sushi_hip_load_histogram.restype = ci
    L.sushi_hip_load_histogram.argtypes = [vp, i64, ci, u32, u32, ci, vp, vp]
    L.sushi_hip_load_normalise.restype = ci
    L.sushi_hip_load_normalise.argtypes = [vp, i64, cf, cf, cf, vp, vp]
    L.sushi_hip_profile_begin.restype = ci
    L.sushi_hip_profile_end.restype = ci
    L.sushi_hip_profile_end.argtypes = [vp, ci, ctypes.POINTER(ci)]
    if L.sushi_hip_abi_version() != ABI_VERSION:
        raise NativeError("libsushi_hip.so ABI version mismatch")
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        msg = lib().sushi_hip_strerror(rc).decode()
        raise NativeError("%s failed: %s (%d)" % (what, msg, rc))


def fft_layout(win_start, n_pos, tmpl_len):
    """(block pairs, pattern segments) of one request on the FFT path (sushi_hip_fft_layout)."""
    a, b = ctypes.c_int32(0), ctypes.c_int32(0)
    check(lib().sushi_hip_fft_layout(int(win_start), int(n_pos), int(tmpl_len), ctypes.byref(a), ctypes.byref(b)),
          "sushi_hip_fft_layout")
    return a.value, b.value


def profile_begin():
    check(lib().sushi_hip_profile_begin(), "sushi_hip_profile_begin")


def profile_end(max_calls):
    """-> float32[n_calls, NSTAGES] milliseconds per stage of every FFT-path call since profile_begin."""
    buf = np.zeros((max(1, max_calls), NSTAGES), np.float32)
    n = ctypes.c_int(0)
    check(lib().sushi_hip_profile_end(buf.ctypes.data, int(max_calls), ctypes.byref(n)), "sushi_hip_profile_end")
    return buf[:n.value]
