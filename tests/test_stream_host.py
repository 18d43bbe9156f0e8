"""Where a prepared stream's parts lie and what a curve or a retime call uploads, on the CPU: sushi_amd/csrc/stream_core.hpp,
curve_core.hpp and the host part of retime_core.hpp (host only) built with g++ into tests/host_stream_check.cpp, which states what
each must give; its --dump against the record (tests/golden/stream_stage.json); and, on the GPU, what the library really answers
and uploads against what the check stages -- the library and the check are the same code."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from host_checks import build_check

HERE = os.path.dirname(os.path.abspath(__file__))
PB, COARSE_G, FFT_N = 4096, 256, 16384
CURVE_HEAD = 256


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("host_stream_check", tmp_path_factory.mktemp("stream_check"))


def _recorded():
    with open(os.path.join(HERE, "golden", "stream_stage.json")) as f:
        return f.read()


def test_every_case_passes_its_checks(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_dump_equals_the_record(check_exe):
    got = subprocess.check_output([check_exe, "--dump"], text=True)
    assert got == _recorded()                                            # byte for byte
    cases = [json.loads(line) for line in got.splitlines()]
    streams = [c for c in cases if c["kind"] == "stream"]
    assert {c["n"] for c in streams} == {1, PB - 1, PB, PB + 1, 3 * COARSE_G + 1, 2 * FFT_N + 7, 347000000}
    assert len(streams) == 7 * 2 * 2 and all(len(c["views"]) == 11 and c["total"] % 256 == 0 for c in streams)
    assert {c["kind"] for c in cases} == {"stream", "curves", "retime"} and all(c["rc"] == 0 for c in cases if c["kind"] != "stream")


def test_checks_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The same program with its own sanitizer runtime, run stand-alone (no environment, no preload): exit 0, nothing on stderr."""
    exe = build_check("host_stream_check", tmp_path, sanitize=True)
    for args in ([], ["--dump"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr


def _samples(rng, n, dtype):
    return rng.integers(0, 256, n, dtype=np.uint8) if dtype == np.uint8 else rng.random(n, dtype=np.float32)


@pytest.mark.gpu
def test_a_stream_s_views_lie_where_the_record_says():
    """A stream of every small length of the record, both sample types, the longest of them searchable (spectra in the tail of its
    own buffer): sushi_hip_stream_bytes is the recorded total and every view is the recorded (offset from the buffer, bytes)."""
    import torch
    from sushi_amd import _native
    from sushi_amd.device import _buffer, _raw_stream, _require_gpu
    L = _native.lib()
    dev = _require_gpu()
    want = {(c["n"], c["dtype"], c["searchable"]): c for c in map(json.loads, _recorded().splitlines()) if c["kind"] == "stream"}
    rng = np.random.default_rng(20261019)
    for n in (1, PB - 1, PB, PB + 1, 3 * COARSE_G + 1, 2 * FFT_N + 7):
        for code, dtype in ((_native.U8, np.uint8), (_native.F32, np.float32)):
            searchable = int(n == 2 * FFT_N + 7)
            rec = want[(n, code, searchable)]
            assert L.sushi_hip_stream_bytes(n, code, searchable) == rec["total"]
            raw = torch.from_numpy(_samples(rng, n, dtype)).to(dev)
            mem = _buffer(rec["total"], dev)
            h = ctypes.c_void_p()
            _native.check(L.sushi_hip_stream_create(raw.data_ptr(), code, n, searchable, mem.data_ptr(), mem.numel(), _raw_stream(dev),
                                                    ctypes.byref(h)), "sushi_hip_stream_create")
            try:
                for which, (off, nbytes) in enumerate(rec["views"]):
                    p, nb = ctypes.c_void_p(), ctypes.c_size_t()
                    _native.check(L.sushi_hip_stream_view(h, which, ctypes.byref(p), ctypes.byref(nb)), "sushi_hip_stream_view")
                    got = (p.value - mem.data_ptr() if p.value else -1, nb.value)
                    assert got == (off, nbytes), (n, code, which)
            finally:
                torch.cuda.synchronize()
                L.sushi_hip_stream_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_a_curve_call_uploads_the_staged_image(check_exe, tmp_path, dtype):
    """Three requests of 1, 256 and 1025 positions: behind the queue head, which the kernel advances, the workspace holds the image
    the host check stages for them, byte for byte."""
    import torch
    from sushi_amd import _native
    from sushi_amd.device import DeviceStream, _buffer, _raw_stream
    L = _native.lib()
    rng = np.random.default_rng(7)
    n_dst, n_src = 5000, 4500
    D, S = DeviceStream(_samples(rng, n_dst, dtype)), DeviceStream(_samples(rng, n_src, dtype))
    req = np.zeros(3, _native.REQUEST_DTYPE)
    req["tmpl_off"], req["win_start"], req["tmpl_len"], req["n_pos"] = [5, 0, 4000], [3, 700, 11], [100, 3000, 77], [1, 256, 1025]
    req.tofile(tmp_path / "three.req")
    subprocess.check_call([check_exe, "--stage-curves", str(tmp_path / "three.req"), str(D.dtype_code), str(n_dst), str(n_src), str(tmp_path / "three.img")])
    image = (tmp_path / "three.img").read_bytes()
    assert len(image) == L.sushi_hip_curve_bytes(req.ctypes.data, 3) == CURVE_HEAD + 256
    mem = _buffer(len(image), D.device)
    mem.fill_(0xA5)
    out = torch.empty(int(req["n_pos"].sum()), dtype=torch.float32, device=D.device)
    _native.check(L.sushi_hip_match_curves(D.handle, S.handle, req.ctypes.data, 3, _native.METHOD_SQDIFF_NORMED, mem.data_ptr(), mem.numel(),
                                           out.data_ptr(), _raw_stream(D.device)), "sushi_hip_match_curves")
    torch.cuda.synchronize()
    assert mem[CURVE_HEAD:].cpu().numpy().tobytes() == image[CURVE_HEAD:]
    assert bool(torch.isfinite(out).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_a_retime_call_uploads_the_staged_table(check_exe, tmp_path, dtype):
    """Two segments whose outputs begin at two different distances from a 16-byte boundary: the workspace holds the table the host
    check stages for that output address, byte for byte."""
    import torch
    from sushi_amd import _native
    from sushi_amd.device import _buffer, _raw_stream, _require_gpu
    L = _native.lib()
    dev = _require_gpu()
    code = _native.U8 if dtype == np.uint8 else _native.F32
    n_in, n_out = 3000, 400
    x = torch.from_numpy(_samples(np.random.default_rng(11), n_in, dtype)).to(dev)
    out = torch.zeros(n_out, dtype=x.dtype, device=dev)
    seg = np.zeros(2, _native.RETIME_SEGMENT_DTYPE)
    seg["in_start"], seg["out_off"], seg["out_len"], seg["num"], seg["den"] = [0, 50], [0, 103], [100, 200], [25, 24], [24, 25]
    seg.tofile(tmp_path / "two.seg")
    subprocess.check_call([check_exe, "--stage-retime", str(tmp_path / "two.seg"), str(code), str(n_in), str(n_out), str(out.data_ptr()),
                           str(tmp_path / "two.img")])
    image = (tmp_path / "two.img").read_bytes()
    assert len(image) == 2 * 48 and L.sushi_hip_retime_bytes(2) == 256
    phases = np.frombuffer(image, "<i4").reshape(2, 12)[:, 10]
    assert phases[0] != phases[1]
    mem = _buffer(256, dev)
    mem.fill_(0xA5)
    _native.check(L.sushi_hip_retime(x.data_ptr(), code, n_in, seg.ctypes.data, 2, out.data_ptr(), n_out, mem.data_ptr(), mem.numel(),
                                     _raw_stream(dev)), "sushi_hip_retime")
    torch.cuda.synchronize()
    assert mem[:len(image)].cpu().numpy().tobytes() == image
    assert bool((mem[len(image):] == 0xA5).all())                        # (nothing behind the table is written)
