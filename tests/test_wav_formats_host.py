"""Float, 32-bit, 8-bit and RF64 WAV files without a GPU: the sample rule's NumPy restatement
(sushi_amd.downmix.samples_from_bytes) against the rule written out one sample at a time and in exact rational arithmetic, the
kernel's own arithmetic header compiled for the CPU (tests/host_pcm_check.cpp, under AddressSanitizer + UBSan), the equalities that
tie every new format to the reference-pinned 16-bit load, the header walk of formats='all' and the unchanged refusals of
formats='reference'.  Every comparison is bitwise."""
import os
import struct
import subprocess

import numpy as np
import pytest

import wav_format_cases as cases
from host_checks import HERE, KERNEL_ARITHMETIC
from sushi_amd import _native, downmix, synth
from sushi_amd.common import SushiError
from sushi_amd.wav import DownmixedWavFile, WavStream


@pytest.fixture(autouse=True)
def host_pipeline(monkeypatch):
    """The NumPy pipeline, whatever the box: it is what this file states (the GPU file compares the GPU pipeline with it)."""
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.data.dtype == b.data.dtype and a.data.shape == b.data.shape and a.data.tobytes() == b.data.tobytes() and \
        (a.sample_count, a.padding_size, a.sample_rate) == (b.sample_count, b.padding_size, b.sample_rate)


# ---------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize("fmt", cases.FORMATS)
def test_samples_from_bytes_is_the_rule_bitwise(fmt):
    for channels, n in ((1, 257), (3, 200)):
        data = cases.random_bytes(n, channels, fmt, seed=channels) + b"\x7f" * (cases.WIDTH[fmt] * channels - 1)   # a cut-off frame: dropped
        got = downmix.samples_from_bytes(data, channels, fmt)
        want = cases.rule_samples(data, channels, fmt)
        assert got.dtype == np.float32 and got.shape == (n, channels)
        assert (_bits(got) == _bits(want)).all()
    if fmt in ("s16", "s24"):
        frames = downmix.frames_from_bytes(data, channels, cases.WIDTH[fmt])
        assert (_bits(got) == _bits(frames.astype(np.float32))).all()


@pytest.mark.parametrize("fmt", ["f32", "f64"])
def test_float_specials_against_exact_arithmetic(fmt):
    """Every planted value: +-0.0, denormals, +-1.0, 1 - 2^-24, above full scale, overflow of the multiply and of the cast, NaNs of
    both signs with payloads, +-inf, float64 values exactly between two float32 neighbours."""
    table, expected, kind = (cases.F32_SPECIAL_BITS, cases.F32_EXPECTED, "<u4") if fmt == "f32" else \
        (cases.F64_SPECIAL_BITS, cases.F64_EXPECTED, "<u8")
    data = np.array(table, dtype=kind).tobytes()
    got = _bits(downmix.samples_from_bytes(data, 1, fmt)).reshape(-1)
    for bits, g in zip(table, got):
        assert int(g) == cases.exact_float_sample(bits, fmt), hex(bits)
        assert int(g) == expected.get(bits, int(g)), hex(bits)
    assert set(expected) <= set(table)
    # seeded bit patterns of every kind, against the exact statement
    rng = np.random.default_rng(7)
    rand = rng.integers(0, 1 << 32, 4000, dtype=np.uint64) if fmt == "f32" else \
        (rng.integers(0, 1 << 32, 4000, dtype=np.uint64) << np.uint64(32)) | rng.integers(0, 1 << 32, 4000, dtype=np.uint64)
    if fmt == "f64":        # exponents around float32's range, where the cast rounds, denormalises and overflows
        rand[:2000] = (rand[:2000] & np.uint64(0x800FFFFFFFFFFFFF)) | (rng.integers(1023 - 170, 1023 + 130, 2000).astype(np.uint64) << np.uint64(52))
    got = _bits(downmix.samples_from_bytes(rand.astype(kind).tobytes(), 1, fmt)).reshape(-1)
    for bits, g in zip(rand, got):
        assert int(g) == cases.exact_float_sample(int(bits), fmt), hex(int(bits))
    # scale_float_samples is the same rule on arrays
    v = np.frombuffer(data, dtype="<f4" if fmt == "f32" else "<f8")
    assert (_bits(downmix.scale_float_samples(v)) == _bits(downmix.samples_from_bytes(data, 1, fmt)).reshape(-1)).all()


def test_restatement_refuses_what_it_does_not_know():
    with pytest.raises(SushiError):
        downmix.samples_from_bytes(b"\0" * 8, 1, "s20")
    with pytest.raises(SushiError):
        downmix.scale_float_samples(np.zeros(3, np.int16))
    with pytest.raises(SushiError):
        downmix.mix_host(np.zeros((3, 2), np.float64), np.ones((1, 2), np.float32))


def test_mean_and_mix_take_float32_samples_and_keep_the_int16_bits():
    rng = np.random.default_rng(3)
    frames = rng.integers(-32768, 32768, (1000, 5)).astype(np.int16)
    w = np.ascontiguousarray(rng.standard_normal((3, 5)), dtype=np.float32)
    assert (_bits(downmix.mean_host(frames)) == _bits(downmix.mean_host(frames.astype(np.float32)))).all()
    assert (_bits(downmix.mix_host(frames, w)) == _bits(downmix.mix_host(frames.astype(np.float32), w))).all()
    # the statement itself, one frame at a time
    s = downmix.samples_from_bytes(cases.float_bytes(300, 3, "f32", seed=4), 3, "f32")
    w = np.array([[0.5, -0.25, 1.0 / 3.0]], np.float32)
    mean, mix = downmix.mean_host(s), downmix.mix_host(s, w)[0]
    for f in range(300):
        m = np.float32(np.float32(s[f, 0] + s[f, 1]) + s[f, 2]) / np.float32(3.0)
        x = np.float32(np.float32(w[0, 0] * s[f, 0]) + np.float32(w[0, 1] * s[f, 1])) + np.float32(w[0, 2] * s[f, 2])
        assert _bits(mean[f]) == _bits(m) and _bits(mix[f]) == _bits(x)
    one = downmix.samples_from_bytes(cases.float_bytes(50, 1, "f64", seed=5), 1, "f64")
    assert (_bits(downmix.mean_host(one)) == _bits(one[:, 0])).all()              # one channel: no division


# ---------------------------------------------------------------------------------------------- the kernel's arithmetic on the CPU
@pytest.fixture(scope="module")
def pcm_check(tmp_path_factory):
    """tests/host_pcm_check.cpp with the flags of every check of a kernel's arithmetic header: -ffp-contract=off, ASan + UBSan."""
    exe = os.path.join(str(tmp_path_factory.mktemp("pcm")), "host_pcm_check")
    subprocess.check_call(["g++"] + KERNEL_ARITHMETIC + [os.path.join(HERE, "host_pcm_check.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("fmt", cases.FORMATS)
@pytest.mark.parametrize("channels,n_out", [(1, 1), (2, 3), (3, 8), (32, 2)])
def test_kernel_arithmetic_equals_the_restatement_bitwise(pcm_check, tmp_path, fmt, channels, n_out):
    n = 301
    data = cases.random_bytes(n, channels, fmt, seed=10 * channels + n_out) + b"\x01"       # one byte behind the last frame: ignored
    w = np.ascontiguousarray(np.random.default_rng(channels).standard_normal((n_out, channels)), dtype=np.float32)
    w[0, 0] = -0.0
    fp, fw = os.path.join(tmp_path, "pcm.bin"), os.path.join(tmp_path, "w.bin")
    open(fp, "wb").write(data)
    open(fw, "wb").write(w.tobytes())
    out = subprocess.run([pcm_check, str(_native.PCM_FORMATS[fmt]), str(channels), str(n_out), fp, fw], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = {}
    for line in out.stdout.splitlines():
        words = line.split()
        k = 2 if words[0] == "mix" else 1
        lines[" ".join(words[:k])] = np.array([int(x, 16) for x in words[k:]], np.uint32)
    samples = downmix.samples_from_bytes(data, channels, fmt)
    assert (lines["samples"] == _bits(samples).reshape(-1)).all()
    assert (lines["mean"] == _bits(downmix.mean_host(samples))).all()
    mix = downmix.mix_host(samples, w)
    assert sorted(lines) == sorted(["samples", "mean"] + ["mix %d" % o for o in range(n_out)])
    for o in range(n_out):
        assert (lines["mix %d" % o] == _bits(mix[o])).all(), o


# ---------------------------------------------------------------------------------------------- the equalities
@pytest.fixture(scope="module")
def renditions(tmp_path_factory):
    """One int16 programme (multiples of 256: an 8-bit file can hold it) per (channels, rate), as a 16-bit file written by the
    project's own writer and as every other format's file."""
    d = str(tmp_path_factory.mktemp("renditions"))
    out = {}
    for channels in (1, 2):
        for rate in (12000, 48000):
            x = cases.programme(int(1.37 * rate), channels, seed=rate + channels, step=256)
            paths = {"s16": os.path.join(d, "s16_%d_%d.wav" % (channels, rate))}
            synth.write_wav(paths["s16"], x if channels > 1 else x[:, 0], rate, channels)
            for k, fmt in enumerate(("s24", "s32", "f32", "f64", "u8")):
                paths[fmt] = os.path.join(d, "%s_%d_%d.wav" % (fmt, channels, rate))
                cases.write_wav(paths[fmt], x, rate, fmt, seed=k, extensible=(k % 2 == 1))
            out[channels, rate] = paths
    return out


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
@pytest.mark.parametrize("rate", [12000, 48000])
@pytest.mark.parametrize("channels", [1, 2])
def test_every_rendition_loads_to_the_16_bit_files_bytes(renditions, oracle, channels, rate, sample_type):
    paths = renditions[channels, rate]
    ref = oracle.load_wav_stream(paths["s16"], sample_rate=12000, sample_type=sample_type)
    default = WavStream(paths["s16"], sample_rate=12000, sample_type=sample_type)
    assert default.data.dtype == ref.data.dtype and default.data.tobytes() == ref.data.tobytes()
    for fmt in ("s16", "s24", "s32", "f32", "f64", "u8"):
        got = WavStream(paths[fmt], sample_rate=12000, sample_type=sample_type, formats="all")
        assert got.data.dtype == ref.data.dtype and got.data.shape == ref.data.shape, fmt
        assert got.data.tobytes() == ref.data.tobytes(), fmt
        assert (got.sample_count, got.padding_size) == (ref.sample_count, ref.padding_size), fmt


# ---------------------------------------------------------------------------------------------- the header walk
RATE = 12000


def _frames(n=90, channels=2, seed=1):
    return cases.programme(n, channels, seed, step=256)


def _file(tmp_path, name, fmt_body, data, **kw):
    path = os.path.join(str(tmp_path), name)
    cases.write_file(path, fmt_body, data, **kw)
    return path


def test_extensible_headers_are_classified_by_their_subformat(tmp_path):
    x = _frames()
    for fmt in cases.FORMATS:
        bits = 8 * cases.WIDTH[fmt]
        body = cases.fmt_chunk(0, 2, RATE, bits, cases.subformat(cases.TAG[fmt]), mask=3)
        f = DownmixedWavFile(_file(tmp_path, fmt + ".wav", body, cases.rendition(x, fmt)), formats="all")
        assert (f.sample_format, f.sample_width, f.frame_size, f.channel_mask) == (fmt, cases.WIDTH[fmt], 2 * cases.WIDTH[fmt], 3)
        assert (f.frames_count, f.frames_available, f.channels_count, f.framerate) == (90, 90, 2, RATE)
        raw = f.read_raw(90)
        assert (f.frames(raw).astype(np.float32) == x.astype(np.float32)).all()
        f.close()
    # valid bits left-justified in a wider container: 20 in 24, 24 in 32 -- by the container's width
    for bits, fmt in ((20, "s24"), (24, "s24"), (12, "s16"), (9, "s16"), (17, "s24"), (25, "s32"), (32, "s32"), (8, "u8")):
        f = DownmixedWavFile(_file(tmp_path, "b.wav", cases.fmt_chunk(1, 2, RATE, bits), cases.rendition(x, fmt)), formats="all")
        assert (f.sample_format, f.sample_width) == (fmt, cases.WIDTH[fmt])
        f.close()
    body = cases.fmt_chunk(0, 2, RATE, 32, cases.subformat(1), valid_bits=24)
    f = DownmixedWavFile(_file(tmp_path, "v.wav", body, cases.rendition(x, "s32")), formats="all")
    assert f.sample_format == "s32"
    f.close()
    # an EXTENSIBLE body too short for a SubFormat: PCM, as today (the mask is read where there is one)
    body = cases.fmt_chunk(0, 2, RATE, 24, cases.subformat(3), mask=3, cb=6)
    assert len(body) == 24
    f = DownmixedWavFile(_file(tmp_path, "short.wav", body, cases.rendition(x, "s24")), formats="all")
    assert (f.sample_format, f.channel_mask) == ("s24", 3)
    f.close()


def test_sample_format_is_set_under_both_settings(tmp_path):
    x = _frames()
    for fmt, want in (("s16", "s16"), ("s24", "s24"), ("s32", None), ("u8", None)):
        path = _file(tmp_path, "r.wav", cases.fmt_chunk(1, 2, RATE, 8 * cases.WIDTH[fmt]), cases.rendition(x, fmt))
        f = DownmixedWavFile(path)
        assert (f.sample_format, f.sample_width, f.formats) == (want, cases.WIDTH[fmt], "reference")
        f.close()
        f = DownmixedWavFile(path, "all")
        assert (f.sample_format, f.sample_width, f.formats) == (fmt, cases.WIDTH[fmt], "all")
        f.close()


def test_old_call_sites_work_on_a_bare_object():
    """_decode, readframes' decode and frames_int16 on an object that has only sample_width and channels_count (built with
    __new__, as existing tests do)."""
    raw = cases.rendition(_frames(), "s24", seed=2)
    f = DownmixedWavFile.__new__(DownmixedWavFile)
    f.sample_width, f.channels_count = 3, 2
    frames = f.frames_int16(raw)
    assert frames.dtype == np.int16 and (frames == _frames()).all()
    assert (_bits(f._decode(raw)) == _bits(downmix.mean_host(_frames()))).all()
    assert f.frames(raw).dtype == np.int16
    f.sample_width = 4
    with pytest.raises(SushiError) as e:
        f._decode(raw)
    assert str(e.value) == "Unsupported sample width: 4"


def test_rf64_and_bw64(tmp_path):
    x = _frames(n=40, channels=2)
    data = cases.rendition(x, "f32")
    body = cases.fmt_chunk(3, 2, RATE, 32)
    junk = [(b"JUNK", 5, b"hello\0"), (b"bext", 4, b"abcd")]
    # ds64 carries the size; the data chunk says 0xFFFFFFFF; chunks in between are skipped
    path = _file(tmp_path, "rf64.wav", body, data, container=b"RF64", data_size32=0xFFFFFFFF, ds64=len(data), junk=junk)
    assert os.path.getsize(path) < 600
    f = DownmixedWavFile(path, "all")
    assert (f.sample_format, f.frames_count, f.frames_available) == ("f32", 40, 40)
    assert (f.frames(f.read_raw(40)) == x.astype(np.float32)).all()
    f.close()
    # BW64 is the same container
    f = DownmixedWavFile(_file(tmp_path, "bw64.wav", body, data, container=b"BW64", data_size32=0xFFFFFFFF, ds64=len(data)), "all")
    assert (f.frames_count, f.frames_available) == (40, 40)
    f.close()
    # RF64 with a plain 32-bit data size: that size counts, not ds64's
    f = DownmixedWavFile(_file(tmp_path, "plain.wav", body, data, container=b"RF64", data_size32=len(data) - 16, ds64=8), "all")
    assert (f.frames_count, f.frames_available) == (38, 38)
    f.close()
    # a ds64 that promises more than the file holds: the header's count stays, the buffers are sized by the file
    f = DownmixedWavFile(_file(tmp_path, "big.wav", body, data, container=b"RF64", data_size32=0xFFFFFFFF, ds64=6 << 30), "all")
    assert (f.frames_count, f.frames_available) == ((6 << 30) // 8, 40)
    f.close()
    # a longer ds64 (a table behind the three sizes) is fine; an odd-sized one is padded
    full = struct.pack("<QQQL", 0, len(data), 0, 1) + b"\0" * 12
    path = os.path.join(str(tmp_path), "table.wav")
    with open(path, "wb") as fh:
        fh.write(b"RF64" + struct.pack("<L", 0xFFFFFFFF) + b"WAVE" + b"ds64" + struct.pack("<L", len(full)) + full +
                 b"fmt " + struct.pack("<L", len(body)) + body + b"data" + struct.pack("<L", 0xFFFFFFFF) + data)
    f = DownmixedWavFile(path, "all")
    assert f.frames_count == 40
    f.close()
    # the stream: the RF64 file loads to what the plain file of the same samples loads to
    long = cases.programme(3 * RATE, 2, seed=5)
    a = os.path.join(str(tmp_path), "a.wav")
    cases.write_wav(a, long, RATE, "f32")
    b = os.path.join(str(tmp_path), "b.wav")
    cases.write_wav(b, long, RATE, "f32", container=b"RF64", data_size32=0xFFFFFFFF, ds64=long.size * 4, junk=junk)
    assert _same(WavStream(a, formats="all"), WavStream(b, formats="all"))


def test_refusals_of_formats_all(tmp_path):
    x = _frames()
    s16 = cases.rendition(x, "s16")

    def refused(name, fmt_body, data=s16, **kw):
        with pytest.raises(SushiError) as e:
            DownmixedWavFile(_file(tmp_path, name, fmt_body, data, **kw), "all")
        return str(e.value)

    # tags and widths outside the table: the message names the tag and the bits
    for tag, bits in ((3, 16), (1, 40), (6, 8), (7, 8), (2, 4), (1, 0), (1, 7), (3, 24), (0x55, 16)):
        msg = refused("t.wav", cases.fmt_chunk(tag, 2, RATE, bits))
        assert "0x%04X" % tag in msg and "%d bits" % bits in msg, msg
    # an unknown GUID, a known format with a foreign tail, a float GUID with an integer width
    msg = refused("g.wav", cases.fmt_chunk(0, 2, RATE, 16, cases.subformat(0x11)))
    assert "0xFFFE" in msg and "16 bits" in msg and cases.subformat(0x11).hex() in msg
    msg = refused("g.wav", cases.fmt_chunk(0, 2, RATE, 16, struct.pack("<H", 1) + b"\x01" * 14))
    assert "0xFFFE" in msg and "16 bits" in msg
    msg = refused("g.wav", cases.fmt_chunk(0, 2, RATE, 16, cases.subformat(3)))
    assert "0xFFFE" in msg and "16 bits" in msg
    # RF64 / BW64: no ds64 before data, a short ds64, another chunk of size 0xFFFFFFFF
    body = cases.fmt_chunk(1, 2, RATE, 16)
    assert refused("r.wav", body, container=b"RF64", data_size32=0xFFFFFFFF) == "Invalid WAV file"
    assert refused("r.wav", body, container=b"BW64") == "Invalid WAV file"
    assert refused("r.wav", body, container=b"RF64", data_size32=0xFFFFFFFF, ds64=len(s16), ds64_size=20) == "Invalid WAV file"
    assert refused("r.wav", body, container=b"RF64", data_size32=0xFFFFFFFF, ds64=len(s16), ds64_size=16) == "Invalid WAV file"
    assert refused("r.wav", body, container=b"RF64", data_size32=0xFFFFFFFF, ds64=len(s16),
                   junk=[(b"JUNK", 0xFFFFFFFF, b"abcd")]) == "Invalid WAV file"
    # ds64 behind the data chunk is never seen
    path = os.path.join(str(tmp_path), "late.wav")
    with open(path, "wb") as fh:
        fh.write(b"RF64" + struct.pack("<L", 0xFFFFFFFF) + b"WAVE" + b"fmt " + struct.pack("<L", len(body)) + body +
                 b"data" + struct.pack("<L", len(s16)) + s16 + b"ds64" + struct.pack("<LQQQL", 28, 0, len(s16), 0, 0))
    with pytest.raises(SushiError) as e:
        DownmixedWavFile(path, "all")
    assert str(e.value) == "Invalid WAV file"
    # other containers stay refused, with today's text
    assert refused("x.wav", body, container=b"RIFX") == "File does not start with RIFF id"
    # a plain RIFF file's placeholder size keeps today's rule: the header's count, the file's frames
    f = DownmixedWavFile(_file(tmp_path, "p.wav", body, s16, data_size32=0xFFFFFFFF), "all")
    assert (f.frames_count, f.frames_available) == (0xFFFFFFFF // 4, 90)
    f.close()
    # the setting itself
    with pytest.raises(SushiError):
        DownmixedWavFile(os.path.join(str(tmp_path), "p.wav"), "everything")


def test_reference_setting_refuses_each_new_file_with_todays_text(tmp_path):
    x = _frames(n=RATE, channels=1)
    files = {"f32": ("unknown format: 3", {}), "f64": ("unknown format: 3", {}), "s32": ("Unsupported sample width: 4", {}),
             "u8": ("Unsupported sample width: 1", {}),
             "s16": ("File does not start with RIFF id", dict(container=b"RF64", data_size32=0xFFFFFFFF, ds64=2 * RATE))}
    for fmt, (text, kw) in files.items():
        path = os.path.join(str(tmp_path), fmt + ".wav")
        cases.write_wav(path, x, RATE, fmt, **kw)
        for call in (lambda: WavStream(path), lambda: WavStream(path, formats="reference"),
                     lambda: WavStream.load_mixes(path, ["mean"]), lambda: WavStream(path, downmix=[1.0])):
            with pytest.raises(SushiError) as e:
                call()
            # (the header's refusals come from the header walk itself; a width is refused where it is decoded, inside the loader)
            assert str(e.value) == (text if "width" not in text else "Error while loading {0}: {1}".format(path, text)), fmt
        assert WavStream(path, formats="all").sample_count == RATE
    # a float file under an EXTENSIBLE header is read as integers' width first, as before: 32 bits are refused by their width
    path = os.path.join(str(tmp_path), "ext.wav")
    cases.write_wav(path, x, RATE, "f32", extensible=True)
    with pytest.raises(SushiError) as e:
        WavStream(path)
    assert str(e.value).endswith("Unsupported sample width: 4")


def test_formats_is_checked_where_the_other_arguments_are(tmp_path):
    missing = os.path.join(str(tmp_path), "missing.wav")
    for call in (lambda **kw: WavStream(missing, **kw), lambda **kw: WavStream.load_mixes(missing, ["mean"], **kw)):
        with pytest.raises(SushiError) as e:
            call(formats="every")
        assert "formats" in str(e.value)
        with pytest.raises(SushiError) as e:
            call(formats=None)
        assert "formats" in str(e.value)
        with pytest.raises(SushiError) as e:
            call(formats="every", sample_type="int16")                  # the order: sample type, resample, formats
        assert "sample type" in str(e.value)
        with pytest.raises(SushiError) as e:
            call(formats="every", resample="cubic")
        assert "resample" in str(e.value)
        with pytest.raises(IOError):
            call(formats="all")                                         # the file is opened after the checks


# ---------------------------------------------------------------------------------------------- with downmix= and resample=
@pytest.mark.parametrize("fmt", ["f32", "s32"])
def test_formats_with_downmix_equals_mix_host(tmp_path, fmt):
    rate = 24000
    n = int(1.2 * rate)
    data2, data6 = cases.random_bytes(n, 2, fmt, seed=21), cases.random_bytes(n, 6, fmt, seed=22)
    two = _file(tmp_path, "two.wav", cases.fmt_chunk(cases.TAG[fmt], 2, rate, 32), data2)
    six = _file(tmp_path, "six.wav", cases.fmt_chunk(0, 6, rate, 32, cases.subformat(cases.TAG[fmt]), mask=0x60F), data6)
    s2, s6 = downmix.samples_from_bytes(data2, 2, fmt), downmix.samples_from_bytes(data6, 6, fmt)
    explicit = [0.25, -1.0, 0.0, 0.70710678, 1.0 / 3.0, -0.0]
    for path, s, mix, mask in ((two, s2, "side", None), (six, s6, "stereo", 0x60F), (six, s6, explicit, 0x60F)):
        w = downmix.weight_matrix([mix], s.shape[1], mask)
        for sample_type in ("uint8", "float32"):
            want = WavStream.from_samples(downmix.mix_host(s, w)[0], rate, sample_type=sample_type)
            got = WavStream(path, sample_type=sample_type, downmix=mix, formats="all")
            assert _same(got, want), (mix, sample_type)
    # load_mixes: one pass, the mean among the mixes
    mean, side = WavStream.load_mixes(two, ["mean", "side"], sample_type="float32", formats="all")
    assert _same(mean, WavStream.from_samples(downmix.mean_host(s2), rate, sample_type="float32"))
    assert _same(side, WavStream(two, sample_type="float32", downmix="side", formats="all"))
    assert _same(mean, WavStream(two, sample_type="float32", formats="all"))


def test_formats_with_fir_resample_equals_resample_host_of_the_restated_samples(tmp_path):
    from sushi_amd.resample import resample_host
    from sushi_amd.row import row_layout
    rate = 48000
    n = int(1.6 * rate)
    data = cases.random_bytes(n, 2, "f32", seed=31)
    path = _file(tmp_path, "fir.wav", cases.fmt_chunk(3, 2, rate, 32), data)
    mono = downmix.mean_host(downmix.samples_from_bytes(data, 2, "f32"))
    got = WavStream(path, sample_type="float32", resample="fir", formats="all")
    assert _same(got, WavStream.from_samples(mono, rate, sample_type="float32", resample="fir"))
    assert not _same(got, WavStream(path, sample_type="float32", formats="all"))
    # the body before the clip: resample_host's samples, wherever the clip left them alone
    lay = row_layout(n, rate, n, 12000, WavStream.READ_CHUNK_SIZE, WavStream.PADDING_SECONDS)
    body = resample_host(mono, rate, 12000, lay.n_body)
    row = np.zeros(lay.total, np.float32)
    row[lay.padding_size:lay.padding_size + lay.n_body] = body
    row[:lay.padding_size], row[lay.total - lay.padding_size:] = row[lay.padding_size], row[lay.total - lay.padding_size - 1]
    hi, lo = float(np.median(row[row >= 0])) * 3, float(np.median(row[row <= 0])) * 3
    want = (np.clip(row, lo, hi) - np.float32(lo)) / np.float32(hi - lo)
    assert (_bits(got.data[0]) == _bits(want)).all()


def test_from_channels_takes_float_frames(tmp_path):
    rate = 12000
    n = 2 * rate
    data = cases.float_bytes(n, 2, "f32", seed=41)
    path = _file(tmp_path, "c.wav", cases.fmt_chunk(3, 2, rate, 32), data)
    frames32 = np.frombuffer(data, dtype="<f4").reshape(n, 2)
    for mix in ("mean", "side", [0.3, 0.9]):
        want = WavStream(path, sample_rate=rate, sample_type="float32", downmix=mix, formats="all")
        assert _same(WavStream.from_channels(frames32, rate, mix, sample_rate=rate, sample_type="float32"), want), mix
    data = cases.float_bytes(n, 3, "f64", seed=42)
    path = _file(tmp_path, "d.wav", cases.fmt_chunk(3, 3, rate, 64), data)
    frames64 = np.frombuffer(data, dtype="<f8").reshape(n, 3)
    for mix in ("mean", [0.5, -0.5, 0.125]):
        want = WavStream(path, sample_rate=rate, sample_type="uint8", downmix=mix, formats="all")
        assert _same(WavStream.from_channels(frames64, rate, mix, sample_rate=rate, sample_type="uint8"), want), mix
    # int16 frames: unchanged; other types: refused
    x = cases.programme(n, 2, seed=43)
    ref = os.path.join(str(tmp_path), "e.wav")
    synth.write_wav(ref, x, rate, 2)
    assert _same(WavStream.from_channels(x, rate, "mean", sample_rate=rate), WavStream(ref, sample_rate=rate))
    with pytest.raises(SushiError):
        WavStream.from_channels(x.astype(np.int32), rate, "mean")


# ---------------------------------------------------------------------------------------------- the entry points' argument checks
def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    cases.check_entry_point_refusals(_native.lib())
    assert _native.PCM_FORMATS == {"u8": 1, "s16": 2, "s24": 3, "s32": 4, "f32": 5, "f64": 6}
    with open(_native.HEADER_PATH) as f:
        text = f.read()
    for name, code in _native.PCM_FORMATS.items():
        assert "#define SUSHI_HIP_PCM_%s %d\n" % (name.upper(), code) in text
