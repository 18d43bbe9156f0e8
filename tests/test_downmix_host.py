"""The weighted downmix without a GPU: the weight tables, the NumPy restatement of sushi_hip_load_decode_mix's
arithmetic (sushi_amd/downmix.py mix_host), the kernel's own arithmetic header compiled for the CPU (tests/host_downmix_check.cpp,
under AddressSanitizer + UBSan), the entry point's argument checks, the loader's host path, and the job it is for: a dub, whose own
speech the side mix removes."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import downmix_cases as cases
from host_checks import build_check
from sushi_amd import _native, downmix
from sushi_amd.common import SushiError
from sushi_amd.wav import DownmixedWavFile, WavStream

F = np.float32
A, B = F(0.70710678), F(0.35355339)


# ---------------------------------------------------------------------------------------------- weights_for
def test_channel_positions():
    assert downmix.channel_positions(1) == ["FC"] and downmix.channel_positions(2) == ["FL", "FR"]
    assert downmix.channel_positions(6) == ["FL", "FR", "FC", "LFE", "BL", "BR"]
    assert downmix.channel_positions(8) == ["FL", "FR", "FC", "LFE", "BL", "BR", "SL", "SR"]
    assert downmix.channel_positions(3) is None and downmix.channel_positions(5) is None
    assert downmix.channel_positions(6, 0x60F) == ["FL", "FR", "FC", "LFE", "SL", "SR"]        # 5.1 with side surrounds
    assert downmix.channel_positions(3, 0x7) == ["FL", "FR", "FC"]
    assert downmix.channel_positions(2, 0x4) is None and downmix.channel_positions(2, 0) is None   # the mask names another count
    assert downmix.channel_positions(2, 0x3) == ["FL", "FR"]


def test_weight_tables():
    def w(mix, ch, mask=None):
        got = downmix.weights_for(mix, ch, mask)
        assert got.dtype == np.float32 and got.shape == (ch,)
        return got.tolist()

    assert w("side", 2) == [0.5, -0.5] and w("side", 2, 0x3) == [0.5, -0.5]
    assert w("stereo", 2) == [0.5, 0.5]
    assert w("no_centre", 2) == [0.5, 0.5]
    assert w("side", 6) == [0.5, -0.5, 0, 0, 0, 0]
    assert w("centre", 6) == [0, 0, 1, 0, 0, 0]
    assert w("no_centre", 6) == [F(0.25), F(0.25), 0, 0, F(0.25), F(0.25)]
    assert w("stereo", 6) == [0.5, 0.5, A, 0, B, B]
    assert w("stereo", 6, 0x60F) == [0.5, 0.5, A, 0, B, B]                 # side surrounds fold down as back ones do
    assert w("stereo", 6, 0x3F) == w("stereo", 6)
    assert w("side", 8) == [0.5, -0.5, 0, 0, 0, 0, 0, 0]
    assert w("centre", 8) == [0, 0, 1, 0, 0, 0, 0, 0]
    assert w("no_centre", 8) == [F(1 / 6)] * 2 + [0, 0] + [F(1 / 6)] * 4
    assert w("stereo", 8) == [0.5, 0.5, A, 0, B, B, B, B]
    assert w("stereo", 8, 0x63F) == w("stereo", 8)
    assert w("centre", 3, 0x7) == [0, 0, 1] and w("no_centre", 3, 0x7) == [0.5, 0.5, 0]
    assert w("centre", 1) == [1.0]
    # a mask reorders nothing but can name other speakers: 0x107 = FL FR FC BC -- BC takes no part in 'stereo'
    assert w("stereo", 4, 0x107) == [0.5, 0.5, A, 0]
    assert w([1, 2, 3], 3) == [1, 2, 3] and w(np.array([0.25, -1.0]), 2) == [0.25, -1.0] and w((0.0,), 1) == [0.0]
    m = downmix.weight_matrix(["side", [1, 0], "stereo"], 2)
    assert m.dtype == np.float32 and m.flags.c_contiguous and m.tolist() == [[0.5, -0.5], [1, 0], [0.5, 0.5]]


def test_weight_errors():
    for mix, ch, mask in (("side", 1, None), ("centre", 2, None), ("stereo", 1, None), ("no_centre", 1, None),
                          ("side", 3, None),                      # three channels without a mask: layout unknown
                          ("side", 2, 0x4), ("centre", 2, 0x3), ("side", 2, 0xC),
                          ([1, 2], 3, None), ([1, 2, 3, 4], 3, None), ([], 1, None),
                          ([1.0, float("nan")], 2, None), ([float("inf"), 0.0], 2, None), ([[1, 2]], 2, None),
                          ("karaoke", 2, None), ("mean", 2, None), (None, 2, None), (0.5, 1, None),
                          ("side", 0, None), ([1.0] * 33, 33, None)):
        with pytest.raises(SushiError):
            downmix.weights_for(mix, ch, mask)
    with pytest.raises(SushiError):
        downmix.weight_matrix([], 2)
    with pytest.raises(SushiError):
        downmix.weight_matrix(["side"] * 9, 2)


def test_extensible_file_gives_back_its_mask(tmp_path):
    frames = cases.random_frames(100, 6, 2, seed=1)
    p = os.path.join(tmp_path, "x.wav")
    cases.write_wav(p, frames, 48000, mask=0x60F)
    f = DownmixedWavFile(p)
    assert f.channel_mask == 0x60F and isinstance(f.channel_mask, int) and f.channels_count == 6 and f.frames_count == 100
    got = f.frames_int16(f.read_raw(100))
    assert got.dtype == np.int16 and (got == frames).all()
    f.close()
    cases.write_wav(p, frames, 48000)
    f = DownmixedWavFile(p)
    assert f.channel_mask is None
    f.close()
    # EXTENSIBLE, but the chunk ends in front of the mask (18 bytes: cbSize 0)
    import struct
    data = cases.pcm_bytes(frames, 2)
    with open(p, "wb") as fh:
        fmt = struct.pack('<HHLLHHH', 0xFFFE, 6, 48000, 48000 * 12, 12, 16, 0)
        fh.write(b'RIFF' + struct.pack('<L', 4 + 8 + len(fmt) + 8 + len(data)) + b'WAVE' + b'fmt ' + struct.pack('<L', len(fmt)) + fmt)
        fh.write(b'data' + struct.pack('<L', len(data)) + data)
    f = DownmixedWavFile(p)
    assert f.channel_mask is None and f.frames_count == 100
    f.close()


# ---------------------------------------------------------------------------------------------- mix_host
def test_mix_host_hand_computed():
    frames = np.array([[-32768, 32767], [32767, -32768], [0, 0], [1, 1], [-3, 5]], np.int16)
    out = downmix.mix_host(frames, np.array([[0.5, -0.5], [0.5, 0.5], [-0.0, 0.0]], np.float32))
    assert out.dtype == np.float32 and out.shape == (3, 5)
    assert out[0].tolist() == [-32767.5, 32767.5, 0.0, 0.0, -4.0]
    assert out[1].tolist() == [-0.5, -0.5, 0.0, 1.0, 1.0]
    # signed zeros fall out of the statement: 0.5 * 0 + -0.5 * 0 = 0 + -0 = +0.0; -0.0 * 32767 + 0.0 * -32768 = -0 + -0 = -0.0; and a
    # single channel keeps its sign
    assert (out[2] == 0).all() and np.signbit(out[2]).tolist() == [False, True, False, False, False] and not np.signbit(out[0][2])
    one = downmix.mix_host(np.array([[0], [5]], np.int16), np.array([[-1.0]], np.float32))
    assert np.signbit(one[0, 0]) and one[0].tolist() == [-0.0, -5.0]
    # every product and every sum rounds to float32: 0.1f * 3 + 0.1f * 3, the way float32 does it
    w = np.array([[0.1, 0.1, 0.7]], np.float32)
    got = downmix.mix_host(np.array([[3, 3, -1]], np.int16), w)[0, 0]
    want = F(F(F(w[0, 0] * F(3)) + F(w[0, 1] * F(3))) + F(w[0, 2] * F(-1)))
    assert got == want and got.dtype == np.float32
    with pytest.raises(SushiError):
        downmix.mix_host(frames, np.ones((1, 3), np.float32))
    with pytest.raises(SushiError):
        downmix.mix_host(frames.astype(np.int32), np.ones((1, 2), np.float32))


@pytest.mark.parametrize("width", [2, 3])
def test_half_half_is_the_mean_of_stereo(tmp_path, width):
    """[0.5, 0.5] against the loader's (a + b) / 2: both are exact on two int16 values, so they agree to the bit."""
    frames = cases.random_frames(5000, 2, width, seed=2)
    p = os.path.join(tmp_path, "s.wav")
    cases.write_wav(p, frames, 12000, width=width)
    f = DownmixedWavFile(p)
    raw = f.read_raw(5000)
    mean = f._decode(raw)
    got = downmix.mix_host(f.frames_int16(raw), np.array([[0.5, 0.5]], np.float32))[0]
    f.close()
    assert got.tobytes() == mean.tobytes()
    if width == 3:
        assert (downmix.frames_from_bytes(raw, 2, 3) == (frames >> 8)).all()            # the top two bytes


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic on the CPU
@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    return build_check("host_downmix_check", tmp_path_factory.mktemp("downmix"))


@pytest.mark.parametrize("width", [2, 3])
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 32])
def test_kernel_arithmetic_equals_mix_host_bitwise(host_check, tmp_path, width, channels):
    n = 3001
    rng = np.random.default_rng(100 * width + channels)
    raw = rng.integers(0, 256, n * channels * width + 1, dtype=np.uint8)        # one byte behind the last frame: ignored
    raw[:channels * width] = 0                                                  # a frame of zeros: the signed-zero cases
    frames = downmix.frames_from_bytes(raw.tobytes(), channels, width)
    assert frames.shape == (n, channels)
    fp, fw, fo = (os.path.join(tmp_path, x) for x in ("pcm.bin", "w.bin", "out.bin"))
    raw.tofile(fp)
    for n_out in (1, 8):
        w = cases.mix_weights(n_out, channels, seed=7 * n_out + channels)
        w.tofile(fw)
        r = subprocess.run([host_check, str(width), str(channels), str(n_out), fp, fw, fo], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.fromfile(fo, dtype=np.float32).reshape(n_out, n)
        want = downmix.mix_host(frames, w)
        assert got.tobytes() == want.tobytes()


# ---------------------------------------------------------------------------------------------- the entry point's checks
def test_entry_point_validates_before_any_hip_call():
    """No call here reaches a launch: each breaks one rule, or has n_frames == 0 (OK without a launch)."""
    L = _native.lib()
    C = ctypes
    P, Q = C.c_void_p(1 << 20), C.c_void_p(2 << 20)                      # never dereferenced
    w_ok = np.full(8 * 32, 0.5, np.float32)

    def call(pcm=P, n_frames=0, channels=2, width=2, w=w_ok, n_out=1, out=Q, stride=None):
        return L.sushi_hip_load_decode_mix(pcm, n_frames, channels, width, None if w is None else w.ctypes.data, n_out, out,
                                           n_frames if stride is None else stride, None)

    assert call() == 0
    assert call(pcm=None) == -1 and call(out=None) == -1 and call(w=None) == -1
    assert call(n_frames=-1, stride=10) == -1
    assert call(channels=0) == -1 and call(channels=-1) == -1 and call(channels=33) == -1
    assert call(channels=1) == 0 and call(channels=32, n_out=8) == 0
    assert call(n_out=0) == -1 and call(n_out=9) == -1 and call(n_out=8) == 0
    assert call(width=1) == -1 and call(width=4) == -1 and call(width=3) == 0
    assert call(n_frames=10, stride=9) == -1 and call(n_frames=0, stride=-1) == -1
    assert call(stride=5) == 0
    for bad in (np.nan, np.inf, -np.inf):
        w = w_ok.copy()
        w[3] = bad
        assert call(w=w, n_out=2) == -1                                    # weights [0, 4) are read
        assert call(w=w, n_out=1) == 0                                     # ... and no others
        assert call(w=w, n_out=1, channels=4) == -1
    assert call(out=C.c_void_p((2 << 20) + 2)) == -2 and call(out=C.c_void_p((2 << 20) + 1)) == -2
    assert call(out=C.c_void_p((2 << 20) + 4)) == 0
    assert call(pcm=C.c_void_p((1 << 20) + 1)) == 0 and call(pcm=C.c_void_p((1 << 20) + 7), width=3) == 0     # any byte alignment
    # a bad argument is EINVAL whatever the alignment
    assert call(out=C.c_void_p((2 << 20) + 2), channels=33) == -1
    assert (_native.MIX_MAX_CHANNELS, _native.MIX_MAX_OUTPUTS) == (32, 8)
    assert "sushi_hip_load_decode_mix" in _native.declared_symbols()
    assert L.sushi_hip_abi_version() == 13


# ---------------------------------------------------------------------------------------------- the loader, host path
@pytest.fixture()
def host_load(monkeypatch):
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")


def _same(a, b):
    return a.data.dtype == b.data.dtype and a.data.shape == b.data.shape and a.data.tobytes() == b.data.tobytes() and \
        (a.sample_count, a.padding_size, a.sample_rate) == (b.sample_count, b.padding_size, b.sample_rate)


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_host_loader(host_load, tmp_path, sample_type):
    rate = 24000
    n = int(11.3 * rate)
    frames = cases.random_frames(n, 6, 3, seed=3) // 4
    p = os.path.join(tmp_path, "six.wav")
    cases.write_wav(p, frames, rate, width=3, mask=0x60F)
    default = WavStream(p, sample_rate=12000, sample_type=sample_type)
    assert _same(WavStream(p, sample_rate=12000, sample_type=sample_type, downmix="mean"), default)
    mixes = ["mean", "stereo", "side", [0, 0, 1, 0, 0, 0], "centre"]
    many = WavStream.load_mixes(p, mixes, sample_rate=12000, sample_type=sample_type)
    assert len(many) == len(mixes) and _same(many[0], default)
    for m, s in zip(mixes, many):
        assert _same(s, WavStream(p, sample_rate=12000, sample_type=sample_type, downmix=m)), m
    assert _same(many[3], many[4]) and not _same(many[1], many[2]) and not _same(many[1], default)
    # ... and the stream is the pipeline run on mix_host's row
    top = (frames >> 8).astype(np.int16)
    row = downmix.mix_host(top, downmix.weight_matrix(["stereo"], 6, 0x60F))[0]
    assert _same(many[1], WavStream.from_samples(row, rate, sample_rate=12000, sample_type=sample_type))
    assert _same(many[1], WavStream.from_channels(top, rate, "stereo", sample_rate=12000, sample_type=sample_type, channel_mask=0x60F))
    assert _same(default, WavStream.from_channels(top, rate, "mean", sample_rate=12000, sample_type=sample_type))
    # patterns cut from a mixed stream are ordinary views of a live stream
    from sushi_amd.wav import _locate
    owner, off, length = _locate(many[2].get_substream(2.0, 3.0))
    assert owner is many[2] and off == many[2].padding_size + 24000 and length == 12000
    with pytest.raises(SushiError):
        WavStream(p, downmix="karaoke")
    with pytest.raises(SushiError):
        WavStream(p, downmix=[1, 2])
    with pytest.raises(SushiError):
        WavStream.load_mixes(p, [])
    with pytest.raises(SushiError):
        WavStream.load_mixes(p, ["side"] * 9)


def test_truncated_file_still_loads(host_load, tmp_path):
    rate = 12000
    frames = cases.random_frames(int(3.5 * rate), 2, 2, seed=4) // 4
    p = os.path.join(tmp_path, "short.wav")
    cases.write_wav(p, frames, rate, claim_frames=5 * rate)             # the header promises 5 s, the file holds 3.5 s
    default = WavStream(p, sample_type="float32")
    side = WavStream(p, sample_type="float32", downmix="side")
    mean, side2 = WavStream.load_mixes(p, ["mean", "side"], sample_type="float32")
    assert _same(mean, default) and _same(side, side2)
    assert side.data.shape == default.data.shape and side.sample_count == 5 * rate
    # the frames that exist are there; what the file lacks is zero before the normalisation, one value after it
    pad = side.padding_size
    body = side.data[0, pad:pad + frames.shape[0]]
    assert len(np.unique(body)) > 1000 and len(np.unique(side.data[0, pad + frames.shape[0]:pad + 5 * rate])) == 1


# ---------------------------------------------------------------------------------------------- the dub, end to end
def test_side_mix_removes_a_dub_s_own_speech(host_load, oracle):
    """DESIGN.md 3.13's dub (downmix_cases.dub_frames), float32 streams through the host pipeline, scores from the oracle.  2 s
    patterns at 12, 20, 31 and 44 s of the source, searched +-2000 samples around the same place in the destination: all are found
    1234 samples on under both mixes; under speech (12 s, 44 s) the mean mix scores >= 0.1 where the side mix scores <= 0.01.
    Measured when the feature was written: mean 0.2508 / 0.4045 under speech, 0.0094 / 0.0103 outside; side 0.0005 .. 0.0006."""
    dst_frames, src_frames, gate = cases.dub_frames()
    rate, m, win = cases.RATE, 2 * cases.RATE, cases.DUB_WINDOW
    scores = {}
    for mix in ("mean", "side"):
        dst = WavStream.from_channels(dst_frames, rate, mix, sample_type="float32")
        src = WavStream.from_channels(src_frames, rate, mix, sample_type="float32")
        assert dst.padding_size == src.padding_size
        pad = dst.padding_size
        for t in cases.DUB_EVENTS:
            s0 = pad + int(t * rate)
            pattern = src.data[:, s0:s0 + m]
            result = oracle.match_template(dst.data[:, s0 - win:s0 + win + m], pattern)
            k = int(result.argmin(axis=1)[0])
            scores[mix, t] = float(result[0, k])
            print("%s mix, pattern at %g s: found %+d samples on, score %.4f" % (mix, t, k - win, scores[mix, t]))
            assert k - win == cases.DUB_OFFSET, (mix, t)
    for t in cases.DUB_EVENTS:
        a = int(t * rate) + cases.DUB_OFFSET
        assert gate[a:a + m].any() == (t in (12.0, 44.0))                         # which patterns hold speech (about half of each)
    for t in (12.0, 44.0):
        assert scores["side", t] <= 0.01 and scores["mean", t] >= 0.1
