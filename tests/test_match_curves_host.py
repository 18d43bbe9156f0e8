"""Whole score curves (sushi_hip_match_curves): the host side of the C ABI -- symbols, types, argument checks before any HIP
call, workspace sizes.  No GPU needed."""
import ctypes

import numpy as np

from sushi_amd import _native

C = ctypes


def _req(n):
    r = np.zeros(max(n, 1), dtype=_native.REQUEST_DTYPE)
    r["tmpl_len"], r["n_pos"] = 10, 100
    return r


def test_curve_symbols_are_declared_exported_and_typed():
    declared = _native.declared_symbols()
    assert "sushi_hip_curve_bytes" in declared and "sushi_hip_match_curves" in declared
    L = _native.lib()
    assert L.sushi_hip_curve_bytes.restype is C.c_size_t and len(L.sushi_hip_curve_bytes.argtypes) == 2
    assert L.sushi_hip_match_curves.restype is C.c_int and len(L.sushi_hip_match_curves.argtypes) == 9
    assert L.sushi_hip_abi_version() == 13


def test_curve_arguments_rejected_before_any_hip_call():
    L = _native.lib()
    r = _req(2)
    fake = C.c_void_p(4096)                 # never dereferenced: every check below fails before the streams are read
    out = C.c_void_p(8192)
    nb = 1 << 20
    assert L.sushi_hip_match_curves(None, fake, r.ctypes.data, 2, 0, fake, nb, out, None) == -1
    assert L.sushi_hip_match_curves(fake, None, r.ctypes.data, 2, 0, fake, nb, out, None) == -1
    assert L.sushi_hip_match_curves(fake, fake, None, 2, 0, fake, nb, out, None) == -1
    assert L.sushi_hip_match_curves(fake, fake, r.ctypes.data, 2, 0, None, nb, out, None) == -1
    assert L.sushi_hip_match_curves(fake, fake, r.ctypes.data, 2, 0, fake, nb, None, None) == -1
    assert L.sushi_hip_match_curves(fake, fake, r.ctypes.data, -1, 0, fake, nb, out, None) == -1
    for method in (-1, 2, 7):
        assert L.sushi_hip_match_curves(fake, fake, r.ctypes.data, 2, method, fake, nb, out, None) == -1
    # nothing to do: no call at all
    assert L.sushi_hip_match_curves(fake, fake, r.ctypes.data, 0, 1, fake, nb, out, None) == 0


def test_curve_workspace_bytes():
    L = _native.lib()
    assert L.sushi_hip_curve_bytes(None, 0) == 0
    assert L.sushi_hip_curve_bytes(_req(1).ctypes.data, 0) == 0
    assert L.sushi_hip_curve_bytes(_req(1).ctypes.data, -3) == 0
    sizes = [L.sushi_hip_curve_bytes(_req(n).ctypes.data, n) for n in (1, 2, 7, 100, 1000, 100000)]
    assert all(s > 0 and s % 256 == 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    # a request table of 24-byte requests has to fit (the device descriptors carry the output offsets besides)
    assert sizes[-1] >= 100000 * 24


def test_curve_python_entry_points_exist():
    from sushi_amd import curves, wav
    assert callable(curves.match_curves)
    assert callable(wav.WavStream.match_template) and callable(wav.WavStream.match_templates)
