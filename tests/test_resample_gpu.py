"""Filtered decimation on the GPU: sushi_hip_load_resample_fir against its NumPy restatement (bit for bit) on every
way the kernel serves a step, 64-bit indexing past its grid, the GPU pipeline with resample='fir' against the host pipeline, the
default left as it was, and the programme at two rates through find_substreams."""
import os

import numpy as np
import pytest

import downmix_cases
import resample_cases as cases
from sushi_amd import _native, resample

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(-7.25)
LEAD, TAIL = 7, 9
# (frame rate, sample rate) -> how the kernel serves the step (sushi_amd/csrc/sushi_resample.hip): outputs per workgroup run,
# where the input span lies, where the table's rows lie
STEPS = [((48000, 12000), "4/1: run 1024, span by phase, one row"),
         ((96000, 12000), "8/1 (W = 143): run 512, span by phase, one row"),
         ((44100, 12000), "147/40: run 512, span as it lies, rows in LDS"),
         ((44100, 8000), "441/80: run 1024, span as it lies, rows in global memory (125 KB)"),
         ((11025, 12000), "147/160: run 1024, span as it lies, rows in LDS"),
         ((8000, 12000), "2/3: run 1024, span as it lies, rows in LDS"),
         ((2400000, 12000), "200/1 (W = 3556): no span in LDS, run 256, input read directly")]
SIZES = (1, 63, 64, 65, 255, 257, 511, 513, 1023, 1025, 10007)          # under and over a wave, a run of 512 and one of 1024; 10 / 20 runs


def _call(x, rates, n_body, pad, total, offset):
    """One call with `x` placed `offset` floats behind a 16-byte boundary, writing [LEAD, LEAD + total) of a buffer of sentinels.
    Returns that whole buffer."""
    import torch
    num, den, W, H = resample.fir_table(*rates)
    raw = torch.zeros(x.shape[0] + offset + 4, dtype=torch.float32, device="cuda")
    assert raw.data_ptr() % 16 == 0
    raw[offset:offset + x.shape[0]] = torch.from_numpy(x).cuda()
    table = torch.from_numpy(np.array(H)).cuda()
    out = torch.full((LEAD + total + TAIL,), float(SENTINEL), dtype=torch.float32, device="cuda")
    rc = _native.lib().sushi_hip_load_resample_fir(raw.data_ptr() + 4 * offset, x.shape[0], num, den, table.data_ptr(), W, n_body, pad,
                                                   total, out.data_ptr() + 4 * LEAD, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return out.cpu().numpy()


@pytest.mark.parametrize("rates,how", STEPS, ids=["%d-%d" % r for r, _ in STEPS])
def test_kernel_equals_resample_host_bitwise(rates, how):
    """Every body length x the input 0 and 4 bytes off a 16-byte boundary, the input as short as the body allows (both ends clamp)
    with a leading run of -0.0 / +0.0: the row is body, zeros and both pads as specified, and the sentinels around it are untouched."""
    num, den, W, _ = resample.fir_table(*rates)
    sizes = SIZES if 2 * W < 1000 else SIZES[:-1]                   # (7112 taps: the restatement of 10007 outputs takes seconds)
    for n_body in sizes:
        n_raw = (n_body - 1) * num // den + 1
        x = cases.int16_noise(n_raw, seed=n_body, leading_zeros=min(n_raw // 2, 3 * W))
        body = resample.resample_host(x, rates[0], rates[1], n_body)
        for offset in (0, 1):
            pad = 5 if n_body % 2 else 0
            gap = 3 if offset else 0                                # zeros behind the body, or the right pad straight from its last sample
            total = 2 * pad + n_body + gap
            want = np.zeros(total, np.float32)
            want[pad:pad + n_body] = body
            if pad:
                want[:pad] = want[pad]
                want[total - pad:] = want[total - pad - 1]
            got = _call(x, rates, n_body, pad, total, offset)
            where = (how, n_body, offset)
            assert got[LEAD:LEAD + total].tobytes() == want.tobytes(), where
            assert (got[:LEAD].view(np.uint32) == SENTINEL.view(np.uint32)).all(), where
            assert got[LEAD + total:].shape == (TAIL,) and (got[LEAD + total:].view(np.uint32) == SENTINEL.view(np.uint32)).all(), where


class _HashedInput(object):
    """The 64-bit test's input as resample_host reads it: frames computed from their index, never held."""
    ndim, dtype = 1, np.dtype(np.float32)

    def __init__(self, n):
        self.shape = (n,)

    def __getitem__(self, index):
        return cases.hash_samples(index)


def test_index_arithmetic_is_64_bit_and_the_grid_strides():
    """441/80 with (n_body - 1) * num > 2^32 and 9571 runs for a grid of 2048.  The input is an integer hash of the index, made on the
    device; the first and the last 4096 outputs and every 9973rd between against the restatement on inputs recomputed on the host."""
    import torch
    rates = (44100, 8000)
    num, den, W, H = resample.fir_table(*rates)
    n_body = 9800000
    assert (n_body - 1) * num > 1 << 32
    n_raw = (n_body - 1) * num // den + 1
    raw = (cases.hash_index(torch.arange(n_raw, dtype=torch.int64, device="cuda")) - 32768).to(torch.float32)
    probe = np.array([0, 1, 12345, n_raw - 1], np.int64)
    assert raw[torch.from_numpy(probe).cuda()].cpu().numpy().tobytes() == cases.hash_samples(probe).tobytes()
    table = torch.from_numpy(np.array(H)).cuda()
    out = torch.empty(n_body, dtype=torch.float32, device="cuda")
    rc = _native.lib().sushi_hip_load_resample_fir(raw.data_ptr(), n_raw, num, den, table.data_ptr(), W, n_body, 0, n_body,
                                                   out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    x = _HashedInput(n_raw)
    for first in (0, n_body - 4096):
        want = resample.resample_host(x, rates[0], rates[1], n_body, first=first, count=4096)
        assert out[first:first + 4096].cpu().numpy().tobytes() == want.tobytes(), first
    picks = np.arange(4096, n_body - 4096, 9973, dtype=np.int64)
    got = out[torch.from_numpy(picks).cuda()].cpu().numpy()
    want = resample.resample_host(x, rates[0], rates[1], n_body, first=4096, count=picks.shape[0], stride=9973)
    assert got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- the loader
def _same(a, b):
    return a.data.dtype == b.data.dtype and a.data.shape == b.data.shape and a.data.tobytes() == b.data.tobytes() and \
        (a.sample_count, a.padding_size, a.sample_rate) == (b.sample_count, b.padding_size, b.sample_rate)


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
@pytest.mark.parametrize("framerate", [48000, 44100])
def test_from_samples_fir_gpu_equals_host(monkeypatch, framerate, sample_type):
    from sushi_amd.wav import WavStream
    x = cases.int16_noise(int(3.37 * framerate), seed=8)
    g = WavStream.from_samples(x, framerate, sample_type=sample_type, resample="fir")
    near = WavStream.from_samples(x, framerate, sample_type=sample_type, resample="nearest")
    default = WavStream.from_samples(x, framerate, sample_type=sample_type)
    assert g._dev_row is not None and g._dev_row.is_cuda
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    h = WavStream.from_samples(x, framerate, sample_type=sample_type, resample="fir")
    assert h._dev_row is None
    assert _same(g, h) and not _same(g, near)
    assert g.device_stream().raw.cpu().numpy().tobytes() == g.data[0].tobytes()
    # the default is untouched: 'nearest' and an omitted resample are one code path and one row, the host pipeline's
    assert _same(near, default) and _same(near, WavStream.from_samples(x, framerate, sample_type=sample_type))
    assert (g.sample_count, g.padding_size, g.data.shape) == (near.sample_count, near.padding_size, near.data.shape)


@pytest.fixture(scope="module")
def stereo24(tmp_path_factory):
    """3.3 s of 48 kHz 24-bit stereo."""
    path = os.path.join(tmp_path_factory.mktemp("resample_wavs"), "stereo24.wav")
    downmix_cases.write_wav(path, downmix_cases.random_frames(int(3.3 * 48000), 2, 3, seed=21) // 4, 48000, width=3)
    return path


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_and_load_mixes_fir_gpu_equal_host(monkeypatch, stereo24, sample_type):
    from sushi_amd import load
    from sushi_amd.wav import WavStream
    monkeypatch.setattr(load, "UPLOAD_CHUNK_BYTES", 300000)
    side = WavStream(stereo24, sample_type=sample_type, resample="fir", downmix="side")
    mean = WavStream(stereo24, sample_type=sample_type, resample="fir")
    mixes = WavStream.load_mixes(stereo24, ["mean", "side", [1.0, 0.0]], sample_type=sample_type, resample="fir")
    plain = WavStream(stereo24, sample_type=sample_type)
    assert _same(plain, WavStream(stereo24, sample_type=sample_type, resample="nearest")) and not _same(plain, mean)
    assert _same(mixes[0], mean) and _same(mixes[1], side) and not _same(mean, side)
    for s in [side, mean] + mixes:
        assert s._dev_row is not None and s.device_stream().raw.cpu().numpy().tobytes() == s.data[0].tobytes()
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    assert _same(side, WavStream(stereo24, sample_type=sample_type, resample="fir", downmix="side"))
    assert _same(mean, WavStream(stereo24, sample_type=sample_type, resample="fir"))
    host_mixes = WavStream.load_mixes(stereo24, ["mean", "side", [1.0, 0.0]], sample_type=sample_type, resample="fir")
    assert all(_same(a, b) for a, b in zip(mixes, host_mixes))


# ---------------------------------------------------------------------------------------------- the case the feature is for
def test_programme_at_two_rates_through_find_substreams(oracle):
    """The CPU test's case (tests/test_resample_host.py) on the GPU: the same index under both loads, and scores within the float32
    gate of the oracle's on the same rows."""
    for mode in ("nearest", "fir"):
        dst, src = cases.programme_streams(mode)
        assert dst._dev_row is not None
        row, true = cases.programme_scores(oracle, dst, src)
        pattern = src.get_substream(cases.PATTERN_START, cases.PATTERN_START + cases.PATTERN_SECONDS)
        score, times = dst.find_substreams([pattern], [cases.PATTERN_START], [cases.WINDOW_SECONDS])
        start_time = cases.PATTERN_START - cases.WINDOW_SECONDS
        index = int(round((times[0] - start_time) * dst.sample_rate))
        want = float(row[true])
        print(mode, index, float(score[0]), want)
        assert index == true == int(row.argmin()) == 42000, mode
        assert abs(float(score[0]) - want) <= 1e-4 * want + 2.5e-7, mode
        assert (want >= 0.2) if mode == "nearest" else (want <= 0.01)
