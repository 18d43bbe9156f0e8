"""The GPU load pipeline (csrc/sushi_load.hip, sushi_amd/load.py) at the sizes and rates the workload has.

resample_pad_kernel, radix_hist_kernel and normalise_kernel run at most 8192 workgroups of 256 threads and stride over
the rest: from STRIDE = 2 097 152 samples on, a thread handles more than one sample.  A 2-hour stream has 86 M.  Here every
kernel is compared past that size -- two whole strides and a ragged third -- and the decode kernel past its own grid; the
file decode is compared over many uploads; the decimation index rule over more rates and rounding edges of the last, partial
chunk; the radix select over crafted populations.  References: the NumPy histogram of tests/load_select_ref.py, np.median,
the host pipeline (WavStream._build_host, which tests/test_host_wav.py and tests/test_wav_init_golden.py pin to the oracle
and to the reference's bytecode) and the goldens of tests/golden/wav_init.json.  Every comparison is exact."""
import functools
import hashlib
import json
import math
import os
import struct
import warnings

import numpy as np
import pytest
import torch

import load_select_ref as ref
import wav_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRIDE = 8192 * 256                    # samples one pass of the capped grid covers (sushi_load.hip grid_for)
LARGE = 2 * STRIDE + 70001             # two whole strides and a ragged third


def _lib():
    from sushi_amd import _native
    return _native.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _host_stream(samples, framerate, sample_rate, sample_type):
    from sushi_amd.wav import WavStream
    w = WavStream.__new__(WavStream)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                  # (the degenerate streams divide 0 by 0, as the reference does)
        w._build_host(np.asarray(samples, np.float32), framerate, len(samples), sample_rate, sample_type)
    return w


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _noise(n, seed):
    """int16 noise as a decoded 16-bit file holds it."""
    return (np.random.default_rng(seed).standard_normal(n) * 3000).astype(np.int16)


# ------------------------------------------------------------------ a. the histogram kernel
@functools.lru_cache(maxsize=None)
def _large_population(kind):
    rng = np.random.default_rng(11)
    if kind == "pcm":
        x = _noise(LARGE, 12).astype(np.float32)
        x[::7] = 0.0
    elif kind == "constant-positive":
        x = np.full(LARGE, 1234.5, np.float32)
    elif kind == "constant-negative":
        x = np.full(LARGE, -77.25, np.float32)
    else:                                                   # +0.0, -0.0 and subnormals of both signs, a third each
        bits = rng.integers(1, 0x00800000, LARGE).astype(np.uint32)
        which = rng.integers(0, 3, LARGE)
        bits[which == 0] = 0
        bits |= rng.integers(0, 2, LARGE).astype(np.uint32) << np.uint32(31)
        x = bits.view(np.float32)
        assert (np.abs(x) < np.finfo(np.float32).tiny).all() and np.signbit(x[x == 0]).any() and (~np.signbit(x[x == 0])).any()
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("kind", ["pcm", "constant-positive", "constant-negative", "zeros-subnormals"])
def test_histogram_kernel_equals_numpy_histogram_past_the_grid(kind):
    x = _large_population(kind)
    assert x.shape[0] == LARGE
    L = _lib()
    data = torch.tensor(x, device="cuda")                   # (a copy: the cached population stays read-only)
    hist = torch.empty(256, dtype=torch.int64, device="cuda")
    for side in (0, 1):
        count = int(((x >= 0) if side == 0 else (x <= 0)).sum())
        for prefix, mask, shift in ref.levels(ref.median_key(x, side)):
            hist.fill_(-1)                                  # the call itself zeroes the bins
            rc = L.sushi_hip_load_histogram(data.data_ptr(), LARGE, side, prefix, mask, shift, hist.data_ptr(), _stream())
            assert rc == 0
            got = hist.cpu().numpy()
            want = ref.histogram(x, side, prefix, mask, shift)
            assert (got == want).all(), (kind, side, hex(prefix), shift, np.flatnonzero(got != want)[:8])
            if shift == 24:
                assert int(got.sum()) == count
            elif count:
                assert int(got.sum()) > 0                   # the prefix is the population's own: the level is not vacuous


# ------------------------------------------------------------------ b. medians on the device
def _device_medians(x):
    from sushi_amd import load
    data = torch.tensor(np.ascontiguousarray(x, np.float32), device="cuda")
    hist = torch.empty(256, dtype=torch.int64, device="cuda")
    return [load._median(_lib(), data, int(x.shape[0]), side, hist, _stream()) for side in (0, 1)]


@pytest.mark.parametrize("name,make", ref.POPULATIONS, ids=ref.POPULATION_IDS)
def test_device_median_equals_numpy_median(name, make):
    x = make()
    want = ref.expected_medians(x)
    got = _device_medians(x)
    assert got[0] == want[0] and got[1] == want[1], (name, got, want)


def test_device_median_equals_numpy_median_past_the_grid():
    x = _large_population("pcm")
    want = ref.expected_medians(x)
    got = _device_medians(x)
    assert got[0] == want[0] and got[1] == want[1], (got, want)


def test_device_median_of_an_empty_side_raises():
    from sushi_amd import SushiError, load
    data = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float32, device="cuda")
    hist = torch.empty(256, dtype=torch.int64, device="cuda")
    assert load._median(_lib(), data, 3, 0, hist, _stream()) == 2.0
    with pytest.raises(SushiError):
        load._median(_lib(), data, 3, 1, hist, _stream())


# ------------------------------------------------------------------ c. the resample kernel against the index rule
def _resample_plan(n_raw, framerate, sample_rate):
    """The arguments sushi_amd.load.build_on_device gives sushi_hip_load_resample for `n_raw` frames of a whole file."""
    from sushi_amd.common import py2_round
    rate = sample_rate / float(framerate)
    sample_count = math.ceil(n_raw / float(framerate) * sample_rate)
    chunk, pad = int(framerate), 10 * framerate
    total = int(20 * framerate + sample_count)
    n_full, rest = divmod(n_raw, chunk)
    nl_full = int(py2_round(chunk * rate))
    nl_rest = int(py2_round(rest * rate)) if rest else 0
    scale_full = 1.0 / (float(nl_full) / float(chunk))
    scale_rest = 1.0 / (float(nl_rest) / float(rest)) if nl_rest > 0 else 0.0
    assert total - 2 * pad >= n_full * nl_full + nl_rest
    return dict(chunk=chunk, nl_full=nl_full, scale_full=scale_full, n_full=n_full, rest=rest, nl_rest=nl_rest,
                scale_rest=scale_rest, pad=pad, total=total)


def _expected_frames(n_raw, framerate, sample_rate):
    """Which frame every position of the padded row is read from (-1: never written), in integers, by the host pipeline's
    rule (WavStream._build_host): per one-second chunk minimum(floor(arange(new_len) * scale_x), len - 1), then both pads
    replicate their neighbour.  Returns (row, positions written inside the pads)."""
    from sushi_amd.common import py2_round
    rate = sample_rate / float(framerate)
    inner = np.full(math.ceil(n_raw / float(framerate) * sample_rate), -1, np.int64)
    pos = 0
    if rate == 1:
        inner[:n_raw] = np.arange(n_raw)
        pos = n_raw
    else:
        n_full, rest = divmod(n_raw, framerate)
        for length, count, start in ((framerate, n_full, 0), (rest, 1 if rest else 0, n_full * framerate)):
            if count == 0 or length == 0:
                continue
            new_length = int(py2_round(length * rate))
            if new_length <= 0:
                continue
            scale_x = 1.0 / (float(new_length) / float(length))
            sx = np.minimum(np.floor(np.arange(new_length, dtype=np.float64) * scale_x).astype(np.int64), length - 1)
            idx = (start + np.arange(count, dtype=np.int64)[:, None] * length + sx[None, :]).reshape(-1)
            inner[pos:pos + idx.shape[0]] = idx
            pos += idx.shape[0]
    pad = 10 * framerate
    return np.concatenate([np.full(pad, inner[0]), inner, np.full(pad, inner[-1])]), pos


def _run_resample(n_raw, framerate, sample_rate, first):
    """The row sushi_hip_load_resample builds from raw[i] = first + i, as integers."""
    assert n_raw + first < 2 ** 24                          # every frame number is an exact float32
    p = _resample_plan(n_raw, framerate, sample_rate)
    raw = torch.from_numpy(np.arange(first, first + n_raw, dtype=np.int64).astype(np.float32)).cuda()
    out = torch.full((p["total"],), -5.0, dtype=torch.float32, device="cuda")
    rc = _lib().sushi_hip_load_resample(raw.data_ptr(), n_raw, p["chunk"], p["nl_full"], p["scale_full"], p["n_full"], p["rest"],
                                        p["nl_rest"], p["scale_rest"], p["pad"], p["total"], out.data_ptr(), _stream())
    assert rc == 0
    got = out.cpu().numpy()
    as_int = got.astype(np.int64)
    assert (as_int.astype(np.float32) == got).all()
    return as_int


def _check_resample(n_raw, framerate, sample_rate, first, written=None):
    row, pos = _expected_frames(n_raw, framerate, sample_rate)
    if written is not None:
        assert pos == written
    want = np.where(row < 0, 0, row + first)                # what is never written is zero
    got = _run_resample(n_raw, framerate, sample_rate, first)
    assert got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (n_raw, framerate, sample_rate, bad[:8], got[bad[:8]], want[bad[:8]])


# 48 -> 12 kHz: the last chunk's `rest` frames become py2_round(rest / 4) samples.  rest 1: none (the row's tail is never
# written, stays zero, and the right pad replicates that zero, as the host does); rest 2: py2_round(0.5) == 1, where Python 3's
# round gives 0; rest 4: one.  `written`: the samples the chunks fill, known by hand.
@pytest.mark.parametrize("first", [0, 1], ids=["from0", "from1"])
@pytest.mark.parametrize("rest,written", [(0, 24000), (1, 24000), (2, 24001), (4, 24001)])
def test_resample_kernel_48k_to_12k_last_chunk_rounding(rest, written, first):
    _check_resample(2 * 48000 + rest, 48000, 12000, first, written)
    if rest == 1:
        row, _ = _expected_frames(2 * 48000 + 1, 48000, 12000)
        assert row[480000 + 24000] == -1 and (row[-480000:] == -1).all() and row.shape[0] == 960000 + 24001


# the other rates, one frame count each with a partial last chunk of 1, 3, 11 or 22050 frames -- and the frame counts at
# which the host pipeline was compared with the oracle (rests of 4 among them)
RATE_CASES = [(44100, 8000, 154350), (22050, 12000, 44101), (96000, 12000, 192011), (11025, 12000, 22051),
              (48000, 16000, 48003), (32000, 12000, 96003), (44100, 12000, 88211),
              (96000, 12000, 192004), (32000, 12000, 96004), (48000, 12000, 96002), (48000, 12000, 144000)]


@pytest.mark.parametrize("first", [0, 1], ids=["from0", "from1"])
@pytest.mark.parametrize("framerate,sample_rate,n_raw", RATE_CASES)
def test_resample_kernel_equals_host_index_rule(framerate, sample_rate, n_raw, first):
    _check_resample(n_raw, framerate, sample_rate, first)


@pytest.mark.parametrize("framerate,sample_rate,n_raw", [(48000, 12000, 276 * 48000 + 2), (12000, 12000, 4030007)])
def test_resample_kernel_equals_host_index_rule_past_the_grid(framerate, sample_rate, n_raw):
    assert _resample_plan(n_raw, framerate, sample_rate)["total"] >= LARGE
    _check_resample(n_raw, framerate, sample_rate, 0)


# ------------------------------------------------------------------ d. end to end at large totals
def _compare_with_host(dev, host):
    assert dev._dev_row is not None                         # the GPU pipeline ran
    assert dev.sample_count == host.sample_count and dev.padding_size == host.padding_size
    assert dev.sample_rate == host.sample_rate
    assert _same_bytes(dev.data, host.data)
    want = host.data[0].tobytes()
    assert dev._dev_row.cpu().numpy().tobytes() == want
    assert dev.device_stream().raw.cpu().numpy().tobytes() == want


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
@pytest.mark.parametrize("framerate,sample_rate,seconds", [(12000, 12000, 420.37), (48000, 12000, 300.37), (44100, 8000, 420.5)])
def test_gpu_load_is_bit_identical_to_host_pipeline_past_the_grid(sample_type, framerate, sample_rate, seconds):
    from sushi_amd.wav import WavStream
    pcm = _noise(int(seconds * framerate), framerate + int(seconds))
    host = _host_stream(pcm, framerate, sample_rate, sample_type)
    assert host.data.shape[1] >= 2 * STRIDE + 1
    assert np.isfinite(host.data).all() and host.data.min() != host.data.max()
    dev = WavStream.from_samples(pcm, framerate, sample_rate=sample_rate, sample_type=sample_type)
    _compare_with_host(dev, host)


# ------------------------------------------------------------------ e. the file decode in many uploads
with open(os.path.join(ROOT, "tests", "golden", "wav_init.json")) as _f:
    GOLDEN = dict((g["case"]["name"], g) for g in json.load(_f)["cases"])
SMALL_UPLOAD = 4099                    # prime: no multiple of any frame size


def _uploads(path, upload_bytes):
    """How many pieces decode_file_on_device cuts the file's data chunk into."""
    from sushi_amd.wav import DownmixedWavFile
    w = DownmixedWavFile(path)
    try:
        per_piece = max(1, upload_bytes // w.frame_size)
        assert upload_bytes % w.frame_size != 0 or upload_bytes > w.frames_available * w.frame_size
        return -(-w.frames_available // per_piece)
    finally:
        w.close()


@pytest.mark.parametrize("name", ["six24-12k-u8", "six24-12k-f32", "ch5-16-12k-f32-100", "stereo16-48k-to-12k-f32",
                                  "ch3-16-12k-f32-102"])
def test_decode_in_many_uploads_equals_reference_bytecode(name, tmp_path, monkeypatch):
    from sushi_amd import load
    from sushi_amd.wav import WavStream
    monkeypatch.setenv("SUSHI_HIP_LOAD", "auto")
    monkeypatch.setattr(load, "UPLOAD_CHUNK_BYTES", SMALL_UPLOAD)
    g = GOLDEN[name]
    c = g["case"]
    blob, _ = wav_cases.wav_bytes(c)
    assert hashlib.sha256(blob).hexdigest() == g["wav_sha256"]
    path = os.path.join(str(tmp_path), name + ".wav")
    with open(path, "wb") as f:
        f.write(blob)
    assert _uploads(path, SMALL_UPLOAD) > 3
    s = WavStream(path, sample_rate=c["sample_rate"], sample_type=c["sample_type"])
    assert s._dev_row is not None
    assert float(s.sample_count) == g["sample_count"] and int(s.padding_size) == g["padding_size"]
    assert list(s.data.shape) == g["shape"] and str(s.data.dtype) == g["dtype"]
    assert hashlib.sha256(np.ascontiguousarray(s.data).tobytes()).hexdigest() == g["data_sha256"]
    assert hashlib.sha256(s.device_stream().raw.cpu().numpy().tobytes()).hexdigest() == g["data_sha256"]


@pytest.mark.parametrize("sample_type", ["float32", "uint8"])
def test_truncated_file_decodes_the_same_in_one_upload_and_in_many(sample_type, tmp_path, monkeypatch):
    """The cut-off copy of tests/test_host_wav.py::test_truncated_and_placeholder_headers_do_not_size_buffers, stereo and long
    enough that its zero tail does not take both medians to zero: the header says 50 s, the file holds 49.3 s and three of the
    four bytes of one more frame.  Device against host, in one upload and in 4099-byte uploads."""
    from sushi_amd import load
    from sushi_amd.wav import DownmixedWavFile, WavStream
    rate, channels = 24000, 2
    rng = np.random.default_rng(31)
    pcm = (rng.standard_normal((50 * rate, channels)) * 3000).astype('<i2')
    data = pcm.tobytes()
    kept = int(49.3 * rate)
    path = os.path.join(str(tmp_path), "cut.wav")
    with open(path, "wb") as f:
        f.write(b'RIFF' + struct.pack('<L', 36 + len(data)) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<LHHLLHH', 16, 1, channels, rate, rate * channels * 2, channels * 2, 16))
        f.write(b'data' + struct.pack('<L', len(data)))                 # the header still says 50 s
        f.write(data[:kept * 4 + 3])                                    # ... and the last frame is cut inside
    w = DownmixedWavFile(path)
    assert w.frames_count == 50 * rate and w.frames_available == kept and w.frame_size == 4
    w.close()
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    host = WavStream(path, sample_rate=12000, sample_type=sample_type)
    assert host._dev_row is None and np.isfinite(host.data).all() and host.data.min() != host.data.max()
    monkeypatch.setenv("SUSHI_HIP_LOAD", "auto")
    assert _uploads(path, load.UPLOAD_CHUNK_BYTES) == 1
    _compare_with_host(WavStream(path, sample_rate=12000, sample_type=sample_type), host)
    monkeypatch.setattr(load, "UPLOAD_CHUNK_BYTES", SMALL_UPLOAD)
    assert _uploads(path, SMALL_UPLOAD) > 3
    _compare_with_host(WavStream(path, sample_rate=12000, sample_type=sample_type), host)


# ------------------------------------------------------------------ f. the decode kernel past its grid
def _host_decode(blob, width, channels):
    from sushi_amd.wav import DownmixedWavFile
    host = DownmixedWavFile.__new__(DownmixedWavFile)
    host.sample_width, host.channels_count, host._file = width, channels, None
    return host._decode(blob)


def _device_decode(blob, n, width, channels):
    pcm = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out = torch.full((n,), np.nan, dtype=torch.float32, device="cuda")
    assert pcm.shape[0] == n * width * channels
    rc = _lib().sushi_hip_load_decode(pcm.data_ptr(), n, channels, width, out.data_ptr(), _stream())
    assert rc == 0
    return out.cpu().numpy()


def test_decode_kernel_past_its_grid():
    """decode_downmix_kernel runs at most 65536 workgroups of 256 threads: from 16 777 216 frames on it strides."""
    n = 65536 * 256 + 70001
    blob = np.random.default_rng(17).integers(0, 256, n * 2, dtype=np.uint8).tobytes()
    want = _host_decode(blob, 2, 1)
    got = _device_decode(blob, n, 2, 1)
    assert want.shape == (n,) and _same_bytes(got, want)


@pytest.mark.parametrize("n", [1, 3])
def test_decode_kernel_few_frames_of_24_bit_five_channels(n):
    blob = np.random.default_rng(18 + n).integers(0, 256, n * 15, dtype=np.uint8).tobytes()
    want = _host_decode(blob, 3, 5)
    got = _device_decode(blob, n, 3, 5)
    assert want.shape == (n,) and _same_bytes(got, want)


# ------------------------------------------------------------------ g. degenerate streams: what happens today
def test_mostly_zero_stream_is_nan_where_the_host_stream_is():
    """More than half of the samples are exact zeros, on both sides of zero: both medians are 0, the range is 0 and the
    float32 row is 0 / 0.  The device row is NaN exactly where the host's is and holds the same bits elsewhere.  (What uint8
    makes of NaN is platform-defined and not compared: that run only has to end with a row of the right size.)"""
    from sushi_amd.wav import WavStream
    x = _noise(60001, 41).astype(np.float32)
    x[np.random.default_rng(42).random(60001) < 0.6] = 0.0
    x[0] = x[-1] = 0.0                                      # both pads replicate an edge sample: they are zeros too
    assert (x == 0).sum() * 2 > x.shape[0] and (x > 0).any() and (x < 0).any()
    host = _host_stream(x, 12000, 12000, "float32")
    dev = WavStream.from_samples(x, 12000, sample_rate=12000, sample_type="float32")
    assert dev._dev_row is not None and dev.data.shape == host.data.shape
    nan = np.isnan(host.data)
    assert nan.any()
    assert (np.isnan(dev.data) == nan).all()
    assert (dev.data.view(np.uint32)[~nan] == host.data.view(np.uint32)[~nan]).all()
    assert (np.isnan(dev._dev_row.cpu().numpy()) == nan[0]).all()
    u8 = WavStream.from_samples(x, 12000, sample_rate=12000, sample_type="uint8")
    assert u8.data.shape == host.data.shape and u8.data.dtype == np.uint8 and u8.sample_count == host.sample_count


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_48k_to_12k_with_one_frame_left_over_equals_host(sample_type):
    """100 s of 48 kHz and one frame more: the last chunk holds one frame, which rounds to no sample at 12 kHz, so the
    stream's last sample is never written, stays zero, and the right pad replicates that zero.  The oracle and the reference
    raise on this file (cv2.resize to a width of 0), so the oracle is no reference here: the host pipeline is, and this pins
    the device to it."""
    from sushi_amd.wav import WavStream
    pcm = _noise(100 * 48000 + 1, 51)
    host = _host_stream(pcm, 48000, 12000, sample_type)
    assert host.sample_count == 1200001 and host.data.shape[1] == 960000 + 1200001
    assert np.isfinite(host.data).all() and host.data.min() != host.data.max()
    assert (host.data[0, -480001:] == host.data[0, -1]).all()           # the unwritten sample and its replicas
    dev = WavStream.from_samples(pcm, 48000, sample_rate=12000, sample_type=sample_type)
    _compare_with_host(dev, host)


def test_stream_without_a_sample_at_or_below_zero():
    """No sample <= 0: np.median of nothing is NaN, so the host pipeline returns a row of NaN; the device pipeline raises
    SushiError instead."""
    from sushi_amd import SushiError
    from sushi_amd.wav import WavStream
    x = (np.abs(_noise(24000, 61)).astype(np.float32) + 1.0)
    host = _host_stream(x, 12000, 12000, "float32")
    assert host.data.shape == (1, 240000 + 24000) and np.isnan(host.data).all()
    with pytest.raises(SushiError):
        WavStream.from_samples(x, 12000, sample_rate=12000, sample_type="float32")
