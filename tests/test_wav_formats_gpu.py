"""Float, 32-bit, 8-bit and RF64 WAV files on the GPU: sushi_hip_load_decode_format and
sushi_hip_load_decode_mix_format against the NumPy restatement (sushi_amd.downmix.samples_from_bytes, mean_host, mix_host) and,
for 16- and 24-bit frames, against the existing entry points; WavStream(path, formats='all') on the GPU against the host pipeline;
one search on a float-loaded pair.  Every comparison is bitwise."""
import os

import numpy as np
import pytest

import downmix_cases
import wav_format_cases as cases
from sushi_amd import _native, downmix

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
GAP = 5
N_FRAMES = (1, 63, 64, 65, 255, 256, 257, 1000, 10007)      # below, at and over a wave and a 256-frame tile; 40 tiles
OFFSETS = (0, 1, 3)                                          # bytes into a 16-byte aligned buffer


def _upload(data, offset):
    """The bytes `data` placed `offset` bytes into a device buffer that ends with them; (the buffer, the address of the bytes)."""
    import torch
    raw = np.frombuffer(data, dtype=np.uint8)
    buf = torch.zeros(raw.shape[0] + offset, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset:] = torch.from_numpy(raw.copy()).cuda()
    return buf, buf.data_ptr() + offset


def _guarded(n_rows, n_frames):
    """An output buffer of sentinels: GAP floats, then n_rows rows n_frames + GAP apart."""
    import torch
    return torch.full((GAP + n_rows * (n_frames + GAP),), float(SENTINEL), dtype=torch.float32, device="cuda")


def _check_rows(out, n_frames, want, where):
    """Row o of the guarded buffer `out` (a float32 ndarray) holds want[o], and every sentinel is untouched."""
    stride = n_frames + GAP
    sentinel = SENTINEL.view(np.uint32)
    assert (out[:GAP].view(np.uint32) == sentinel).all(), where
    for o in range(len(want)):
        row = out[GAP + o * stride:GAP + o * stride + n_frames]
        gap = out[GAP + o * stride + n_frames:GAP + (o + 1) * stride]
        assert row.tobytes() == np.ascontiguousarray(want[o], dtype=np.float32).tobytes(), where + (o,)
        assert gap.shape == (GAP,) and (gap.view(np.uint32) == sentinel).all(), where + (o,)


# ---------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8, 32])
@pytest.mark.parametrize("fmt", cases.FORMATS)
def test_both_entry_points_equal_the_restatement_bitwise(fmt, channels):
    """Per n_frames and byte offset of the PCM: the mean entry (channels up to 8) and the mix entry at n_out 1, 3 and 8, rows
    n_frames + 5 apart in a buffer of sentinels.  The float files carry every planted special (wav_format_cases), denormals among
    them: a build that flushes them would differ."""
    import torch
    L = _native.lib()
    st = torch.cuda.current_stream().cuda_stream
    code = _native.PCM_FORMATS[fmt]
    for n_frames in N_FRAMES:
        data = cases.random_bytes(n_frames, channels, fmt, seed=1000 * code + 10 * channels + n_frames % 7)
        samples = downmix.samples_from_bytes(data, channels, fmt)
        assert samples.shape == (n_frames, channels)
        if fmt in ("f32", "f64") and n_frames * channels >= 64:
            assert (np.abs(samples[samples != 0]) < 1e-38).any()                       # a denormal is among the values
        mean = downmix.mean_host(samples)
        weights = [downmix_cases.mix_weights(n_out, channels, seed=n_frames + n_out) for n_out in (1, 3, 8)]
        mixes = [downmix.mix_host(samples, w) for w in weights]
        for offset in OFFSETS:
            buf, pcm = _upload(data, offset)
            if channels <= 8:
                out = _guarded(1, n_frames)
                rc = L.sushi_hip_load_decode_format(pcm, n_frames, channels, code, out.data_ptr() + 4 * GAP, st)
                assert rc == 0, rc
                _check_rows(out.cpu().numpy(), n_frames, [mean], (n_frames, offset, "mean"))
            for w, want in zip(weights, mixes):
                out = _guarded(w.shape[0], n_frames)
                rc = L.sushi_hip_load_decode_mix_format(pcm, n_frames, channels, code, w.ctypes.data, w.shape[0],
                                                        out.data_ptr() + 4 * GAP, n_frames + GAP, st)
                assert rc == 0, rc
                _check_rows(out.cpu().numpy(), n_frames, want, (n_frames, offset, w.shape[0]))
            del buf


def test_a_thread_takes_a_second_frame_of_the_grid_stride_loop():
    """65536 * 256 + 1 mono 8-bit frames: one more than the capped grid has threads."""
    import torch
    L = _native.lib()
    n = 65536 * 256 + 1
    g = torch.Generator(device="cuda").manual_seed(11)
    pcm = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.full((n + GAP,), float(SENTINEL), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert L.sushi_hip_load_decode_format(pcm.data_ptr(), n, 1, _native.PCM_FORMATS["u8"], out.data_ptr(), st) == 0
    want = ((pcm.to(torch.int32) - 128) * 256).to(torch.float32)
    assert torch.equal(out[:n].view(torch.int32), want.view(torch.int32))
    assert (out[n:].cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()
    # the ends of the run against the restatement itself
    for lo in (0, n - 1000):
        got = out[lo:lo + 1000].cpu().numpy()
        assert got.tobytes() == downmix.samples_from_bytes(pcm[lo:lo + 1000].cpu().numpy().tobytes(), 1, "u8")[:, 0].tobytes()
    w = np.array([[-0.5]], np.float32)
    rows = torch.full((n + GAP,), float(SENTINEL), dtype=torch.float32, device="cuda")
    assert L.sushi_hip_load_decode_mix_format(pcm.data_ptr(), n, 1, _native.PCM_FORMATS["u8"], w.ctypes.data, 1, rows.data_ptr(),
                                              n + GAP, st) == 0
    assert torch.equal(rows[:n].view(torch.int32), (want * -0.5).view(torch.int32))
    assert (rows[n:].cpu().numpy().view(np.uint32) == SENTINEL.view(np.uint32)).all()


@pytest.mark.parametrize("fmt", ["s16", "s24"])
@pytest.mark.parametrize("channels", [1, 2, 6])
def test_s16_and_s24_equal_the_existing_entry_points_bitwise(fmt, channels):
    import torch
    L = _native.lib()
    st = torch.cuda.current_stream().cuda_stream
    width, code = cases.WIDTH[fmt], _native.PCM_FORMATS[fmt]
    for n in (257, 100003):
        data = cases.random_bytes(n, channels, fmt, seed=n + channels)
        w = downmix_cases.mix_weights(8, channels, seed=n)
        for offset in (0, 1):
            buf, pcm = _upload(data, offset)
            old, new = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
            assert L.sushi_hip_load_decode(pcm, n, channels, width, old.data_ptr(), st) == 0
            assert L.sushi_hip_load_decode_format(pcm, n, channels, code, new.data_ptr(), st) == 0
            assert torch.equal(old.view(torch.int32), new.view(torch.int32))
            old, new = torch.empty((8, n), dtype=torch.float32, device="cuda"), torch.empty((8, n), dtype=torch.float32, device="cuda")
            assert L.sushi_hip_load_decode_mix(pcm, n, channels, width, w.ctypes.data, 8, old.data_ptr(), n, st) == 0
            assert L.sushi_hip_load_decode_mix_format(pcm, n, channels, code, w.ctypes.data, 8, new.data_ptr(), n, st) == 0
            assert torch.equal(old.view(torch.int32), new.view(torch.int32))
            del buf


def test_entry_points_refuse_bad_arguments():
    cases.check_entry_point_refusals(_native.lib())


# ---------------------------------------------------------------------------------------------- the loader
def _same(a, b):
    return a.data.dtype == b.data.dtype and a.data.shape == b.data.shape and a.data.tobytes() == b.data.tobytes() and \
        (a.sample_count, a.padding_size, a.sample_rate) == (b.sample_count, b.padding_size, b.sample_rate)


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
@pytest.mark.parametrize("fmt,channels", [("u8", 2), ("s32", 3), ("f32", 2), ("f64", 3)])
def test_wavstream_formats_all_gpu_equals_host(tmp_path, monkeypatch, fmt, channels, sample_type):
    """1.3 s at 16 kHz uploaded 1000 bytes at a time: 42 to 500 chunks, whose size is a multiple of the frame size only for the
    8-bit and the float32 file; the mean, a weighted and filtered load, and load_mixes with both."""
    from sushi_amd import load
    from sushi_amd.wav import WavStream
    rate, n = 16000, 20800
    path = os.path.join(str(tmp_path), "in.wav")
    cases.write_file(path, cases.fmt_chunk(cases.TAG[fmt], channels, rate, 8 * cases.WIDTH[fmt]), cases.random_bytes(n, channels, fmt, seed=3))
    mix = [0.5, -0.5, 0.25][:channels]
    monkeypatch.setattr(load, "UPLOAD_CHUNK_BYTES", 1000)
    kw = dict(sample_rate=12000, sample_type=sample_type, formats="all")
    g_mean, g_mix = WavStream(path, **kw), WavStream(path, downmix=mix, resample="fir", **kw)
    g_both = WavStream.load_mixes(path, ["mean", mix, "mean"], **kw)
    assert g_mean._dev_row is not None and g_mean._dev_row.is_cuda and g_mix._dev_row is not None
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    h_mean, h_mix = WavStream(path, **kw), WavStream(path, downmix=mix, resample="fir", **kw)
    assert h_mean._dev_row is None
    assert _same(g_mean, h_mean) and _same(g_mix, h_mix) and not _same(g_mean, g_mix)
    assert g_mean._dev_row.cpu().numpy().tobytes() == h_mean.data.tobytes()
    assert _same(g_both[0], h_mean) and _same(g_both[2], h_mean)
    assert _same(g_both[1], WavStream(path, downmix=mix, **kw))


def test_rf64_file_gpu_equals_host(tmp_path, monkeypatch):
    from sushi_amd import load
    from sushi_amd.wav import WavStream
    rate = 12000
    x = cases.programme(2 * rate, 2, seed=8)
    plain, rf64 = os.path.join(str(tmp_path), "plain.wav"), os.path.join(str(tmp_path), "rf64.wav")
    cases.write_wav(plain, x, rate, "f32")
    cases.write_wav(rf64, x, rate, "f32", container=b"RF64", data_size32=0xFFFFFFFF, ds64=x.size * 4, junk=[(b"JUNK", 3, b"abc\0")])
    monkeypatch.setattr(load, "UPLOAD_CHUNK_BYTES", 50000)
    g = WavStream(rf64, sample_type="float32", formats="all")
    assert g._dev_row is not None and _same(g, WavStream(plain, sample_type="float32", formats="all"))
    # the float file of an int16 programme is the 16-bit file's stream (the default, reference-pinned path)
    s16 = os.path.join(str(tmp_path), "s16.wav")
    cases.write_wav(s16, x, rate, "s16")
    assert _same(g, WavStream(s16, sample_type="float32"))
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    assert _same(g, WavStream(rf64, sample_type="float32", formats="all"))


def test_from_channels_float_frames_gpu_equals_host(monkeypatch):
    from sushi_amd.wav import WavStream
    rate, n = 12000, 24000
    frames = np.frombuffer(cases.float_bytes(n, 2, "f64", seed=9), dtype="<f8").reshape(n, 2).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        both = (frames, frames.astype(np.float32))
    g = [WavStream.from_channels(f, rate, "side", sample_rate=rate, sample_type="float32") for f in both]
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    h = [WavStream.from_channels(f, rate, "side", sample_rate=rate, sample_type="float32") for f in both]
    assert _same(g[0], h[0]) and _same(g[1], h[1])


def test_find_substreams_on_a_float_loaded_pair_returns_the_planted_offset(tmp_path):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    rate, offset = 12000, 3210
    dst_pcm = synth.make_dst_pcm(40, rate, seed=21)
    src_pcm = synth.make_src_pcm(dst_pcm, offset, seed=22)
    pd, ps = os.path.join(str(tmp_path), "dst.wav"), os.path.join(str(tmp_path), "src.wav")
    cases.write_wav(pd, dst_pcm[:, None], rate, "f32")
    cases.write_wav(ps, src_pcm[:, None], rate, "f32", extensible=True, mask=4)
    dst = WavStream(pd, sample_rate=rate, sample_type="float32", formats="all")
    src = WavStream(ps, sample_rate=rate, sample_type="float32", formats="all")
    starts = [5.0, 17.5]
    patterns = [src.get_substream(t, t + 2.5) for t in starts]
    scores, times = dst.find_substreams(patterns, [t + 0.2 for t in starts], [1.5, 1.5])
    for t, score, found in zip(starts, scores, times):
        print("pattern at %g s: found %.6f score %.6f" % (t, found, float(score)))
        assert abs(found - (t + offset / float(rate))) <= 0.5 / rate
