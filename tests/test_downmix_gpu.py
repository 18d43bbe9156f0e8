"""The weighted downmix on the GPU: sushi_hip_load_decode_mix against its NumPy restatement and against the
existing decode (bit for bit), WavStream(downmix=...) / load_mixes GPU pipeline against host pipeline, and the dub the feature is
for: the side mix finds every event and compare_mixes names it."""
import os

import numpy as np
import pytest

import downmix_cases as cases
from sushi_amd import _native, downmix

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
GAP = 5


def _decode_mix(raw, n_frames, channels, width, w, offset):
    """One call on `raw` (uint8 ndarray) placed `offset` bytes into a device buffer; rows out_stride = n_frames + 5 apart in a
    buffer of sentinels.  Returns the whole output buffer (float32 ndarray) and the index of row 0."""
    import torch
    L = _native.lib()
    n_out = w.shape[0]
    buf = torch.zeros(raw.shape[0] + offset + 1, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[offset:offset + raw.shape[0]] = torch.from_numpy(raw).cuda()
    stride = n_frames + GAP
    out = torch.full((GAP + n_out * stride,), float(SENTINEL), dtype=torch.float32, device="cuda")
    rc = L.sushi_hip_load_decode_mix(buf.data_ptr() + offset, n_frames, channels, width, w.ctypes.data, n_out,
                                     out.data_ptr() + 4 * GAP, stride, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return out.cpu().numpy(), GAP


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("width", [2, 3])
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8, 32])
def test_decode_mix_equals_mix_host_bitwise(width, channels):
    """n_out 1, 3, 8 x n_frames 1 .. 10007 (below, at and over a wave and a 256-frame tile; 40 tiles) x the PCM 0, 1 and 7 bytes
    off a 16-byte boundary: every row equals mix_host's, and the sentinels before, between and after the rows are untouched."""
    fs = channels * width
    rng = np.random.default_rng(1000 * width + channels)
    for n_frames in (1, 63, 64, 65, 255, 257, 10007):
        raw = rng.integers(0, 256, n_frames * fs, dtype=np.uint8)
        raw[:fs] = 0                                               # a frame of zeros: the signed-zero cases
        frames = downmix.frames_from_bytes(raw.tobytes(), channels, width)
        for n_out in (1, 3, 8):
            w = cases.mix_weights(n_out, channels, seed=n_frames + n_out)
            want = downmix.mix_host(frames, w)
            for offset in (0, 1, 7):
                got, first = _decode_mix(raw, n_frames, channels, width, w, offset)
                stride = n_frames + GAP
                where = (n_frames, n_out, offset)
                assert (got[:first].view(np.uint32) == SENTINEL.view(np.uint32)).all(), where
                for o in range(n_out):
                    row = got[first + o * stride:first + o * stride + n_frames]
                    gap = got[first + o * stride + n_frames:first + (o + 1) * stride]
                    assert row.tobytes() == want[o].tobytes(), where + (o,)
                    assert gap.shape == (GAP,) and (gap.view(np.uint32) == SENTINEL.view(np.uint32)).all(), where + (o,)


def test_half_half_equals_the_existing_decode_bitwise():
    import torch
    L = _native.lib()
    n = 100003
    raw = np.random.default_rng(5).integers(0, 256, n * 4, dtype=np.uint8)
    w = np.array([[0.5, 0.5]], np.float32)
    got, first = _decode_mix(raw, n, 2, 2, w, 0)
    pcm = torch.from_numpy(raw).cuda()
    mono = torch.empty(n, dtype=torch.float32, device="cuda")
    assert L.sushi_hip_load_decode(pcm.data_ptr(), n, 2, 2, mono.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert got[first:first + n].tobytes() == mono.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------- the loader
def _same(a, b):
    return a.data.dtype == b.data.dtype and a.data.shape == b.data.shape and a.data.tobytes() == b.data.tobytes() and \
        (a.sample_count, a.padding_size, a.sample_rate) == (b.sample_count, b.padding_size, b.sample_rate)


@pytest.fixture(scope="module")
def wav_files(tmp_path_factory):
    """3.3 s of 48 kHz 24-bit stereo and of 6-channel 16-bit (EXTENSIBLE, side surrounds)."""
    d = tmp_path_factory.mktemp("downmix_wavs")
    n = int(3.3 * 48000)
    stereo24, six16 = os.path.join(d, "stereo24.wav"), os.path.join(d, "six16.wav")
    cases.write_wav(stereo24, cases.random_frames(n, 2, 3, seed=11) // 4, 48000, width=3)
    cases.write_wav(six16, cases.random_frames(n, 6, 2, seed=12) // 4, 48000, width=2, mask=0x60F)
    return {"stereo24": stereo24, "six16": six16}


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
@pytest.mark.parametrize("name,mix", [("stereo24", "side"), ("six16", "stereo")])
def test_wavstream_downmix_gpu_equals_host(monkeypatch, wav_files, sample_type, name, mix):
    from sushi_amd import load
    from sushi_amd.wav import WavStream
    path = wav_files[name]
    monkeypatch.setattr(load, "UPLOAD_CHUNK_BYTES", 200000)                   # 0.95 MB / 1.9 MB of PCM: 5 / 10 chunks
    g = WavStream(path, sample_rate=12000, sample_type=sample_type, downmix=mix)
    assert g._dev_row is not None and g._dev_row.is_cuda
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    h = WavStream(path, sample_rate=12000, sample_type=sample_type, downmix=mix)
    assert h._dev_row is None
    assert _same(g, h)
    assert g._dev_row.cpu().numpy().tobytes() == h.data.tobytes()
    assert g.data.shape[1] == 2 * 10 * 48000 + h.sample_count and h.sample_count in (39600, 39601)       # (3.3 s at 12 kHz)


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_load_mixes_equals_single_loads(monkeypatch, wav_files, sample_type):
    from sushi_amd import load
    from sushi_amd.wav import WavStream
    path = wav_files["stereo24"]
    before = WavStream(path, sample_type=sample_type)
    monkeypatch.setattr(load, "UPLOAD_CHUNK_BYTES", 300000)
    mean, side = WavStream.load_mixes(path, ["mean", "side"], sample_type=sample_type)
    assert _same(mean, WavStream(path, sample_type=sample_type)) and _same(mean, before)      # the default load is what it was
    assert _same(side, WavStream(path, sample_type=sample_type, downmix="side"))
    assert _same(side, WavStream(path, sample_type=sample_type, downmix=[0.5, -0.5])) and not _same(side, mean)
    assert side._dev_row is not None and side.device_stream().raw.cpu().numpy().tobytes() == side.data.tobytes()
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    assert _same(mean, WavStream(path, sample_type=sample_type))


# ---------------------------------------------------------------------------------------------- the dub
def test_dub_side_mix_finds_every_event_and_compare_mixes_names_it(tmp_path, oracle):
    """downmix_cases.dub_frames as two stereo WAVs, loaded once each with ['mean', 'side'] (float32): find_substreams on the side
    streams finds all four events 1234 samples on with the oracle's scores, and compare_mixes puts 'side' first."""
    from sushi_amd.wav import WavStream
    dst_frames, src_frames, _gate = cases.dub_frames()
    rate = cases.RATE
    pd, ps = os.path.join(tmp_path, "dst.wav"), os.path.join(tmp_path, "src.wav")
    cases.write_wav(pd, dst_frames, rate)
    cases.write_wav(ps, src_frames, rate)
    names = ["mean", "side"]
    dst = WavStream.load_mixes(pd, names, sample_rate=rate, sample_type="float32")
    src = WavStream.load_mixes(ps, names, sample_rate=rate, sample_type="float32")
    d, s = dst[1], src[1]
    # the same frames from memory: the same streams
    assert _same(d, WavStream.from_channels(dst_frames, rate, "side", sample_rate=rate, sample_type="float32"))
    assert _same(dst[0], WavStream.from_channels(dst_frames, rate, "mean", sample_rate=rate, sample_type="float32"))
    patterns = [s.get_substream(t, t + 2.0) for t in cases.DUB_EVENTS]
    window = cases.DUB_WINDOW / float(rate)
    scores, times = d.find_substreams(patterns, list(cases.DUB_EVENTS), [window] * len(patterns))
    odst = oracle.OracleWavStream(d.data, d.sample_rate, d.sample_count, d.padding_size)
    for p, t, score, found in zip(patterns, cases.DUB_EVENTS, scores, times):
        rs, rt = odst.find_substream(p, t, window)
        print("event at %g s: found %.6f oracle %.6f score %.6f oracle %.6f" % (t, found, rt, float(score), float(rs)))
        assert found == rt and abs(found - (t + cases.DUB_OFFSET / float(rate))) <= 0.5 / rate
        assert abs(float(score) - float(rs)) <= 1e-4 * float(rs) + 2.5e-7          # (the exact stages against cv2's operation order)
        assert float(score) <= 0.01
    ranked = downmix.compare_mixes(src, dst, names)
    print("compare_mixes:", ranked)
    assert [n for n, _ in ranked] == ["side", "mean"] and ranked[0][1] <= 0.01 < ranked[1][1]
    assert ranked == downmix.rank_mixes(names, [[ranked[1][1]], [ranked[0][1]]])
