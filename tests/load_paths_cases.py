"""Shared by tests/test_load_paths.py and tests/golden/gen_load_paths_golden.py (TEST INFRASTRUCTURE): every way a WavStream
comes into being, on a handful of small files, as a digest of what it holds.

The inputs are two seconds and 1237 frames of noise (a last chunk shorter than a second, two chunk boundaries before it), made
from resample_cases.hash_index alone -- integer arithmetic, no library random stream -- and written by downmix_cases.write_wav.
"""
import hashlib
import os
from fractions import Fraction

import numpy as np

import downmix_cases
import resample_cases

SECONDS, EXTRA_FRAMES = 2, 1237
SAMPLE_TYPES = ("uint8", "float32")
RESAMPLE_MODES = ("nearest", "fir")
UPLOAD_BYTES = 200000          # what the GPU test sets load.UPLOAD_CHUNK_BYTES to
SPEED = Fraction(25, 24)

# name -> frame rate, channels, bytes per sample, dwChannelMask (None: a plain PCM header), frames the header claims beyond the file's
INPUTS = {
    "stereo24-48k": dict(rate=48000, channels=2, width=3, mask=None, overclaim=0, seed=1),
    "six16-44k1": dict(rate=44100, channels=6, width=2, mask=0x60F, overclaim=0, seed=2),
    "mono16-12k": dict(rate=12000, channels=1, width=2, mask=None, overclaim=0, seed=3),          # downsample_rate == 1
    "stereo16-48k-short": dict(rate=48000, channels=2, width=2, mask=0x3, overclaim=48000, seed=4),   # the header says a second more
}
CONSTRUCTORS = ("init-mean", "init-side", "load_mixes", "from_samples", "from_channels-mean", "from_channels-weighted", "retimed")


def weights(channels):
    """One explicit weight per channel: both signs, none of them dyadic."""
    return [((c * 7 + 3) % 11 - 5) / 7.0 for c in range(channels)]


def frames_of(name):
    """int [n, C] over the whole range of the input's sample width."""
    c = INPUTS[name]
    n = SECONDS * c["rate"] + EXTRA_FRAMES
    idx = np.arange(n * c["channels"], dtype=np.int64) + c["seed"] * 1000003
    v = resample_cases.hash_index(idx) - 32768
    if c["width"] == 3:
        v = v * 256 + (resample_cases.hash_index(idx + 77777) & 0xFF)
    return v.reshape(n, c["channels"])


def write_input(directory, name):
    """Writes the input; returns (path, int16 frames [n, C] as the loader decodes them, frame rate)."""
    c = INPUTS[name]
    frames = frames_of(name)
    path = os.path.join(str(directory), name + ".wav")
    downmix_cases.write_wav(path, frames, c["rate"], width=c["width"], mask=c["mask"],
                            claim_frames=frames.shape[0] + c["overclaim"] if c["overclaim"] else None)
    top = (frames >> 8 if c["width"] == 3 else frames).astype(np.int16)
    return path, top, c["rate"]


def construct(how, path, top, rate, sample_type, resample):
    """The streams of constructor `how` (a list; load_mixes gives three)."""
    from sushi_amd.wav import WavStream
    kw = dict(sample_rate=12000, sample_type=sample_type, resample=resample)
    w = weights(top.shape[1])
    if how == "init-mean":
        return [WavStream(path, **kw)]
    if how == "init-side":
        return [WavStream(path, downmix="side", **kw)]
    if how == "load_mixes":
        return WavStream.load_mixes(path, ["mean", "side", w], **kw)
    if how == "from_samples":
        return [WavStream.from_samples(top[:, 0], rate, **kw)]
    if how == "from_channels-mean":
        return [WavStream.from_channels(top, rate, "mean", **kw)]
    if how == "from_channels-weighted":
        return [WavStream.from_channels(top, rate, w, **kw)]
    if how == "retimed":
        return [WavStream(path, **kw).retimed(SPEED)]
    raise ValueError(how)


def record(stream):
    d = stream.data
    return {"sha256": hashlib.sha256(np.ascontiguousarray(d).tobytes()).hexdigest(), "shape": list(d.shape), "dtype": str(d.dtype),
            "sample_count": float(stream.sample_count), "padding_size": int(stream.padding_size), "sample_rate": int(stream.sample_rate)}


def outcome(how, path, top, rate, sample_type, resample):
    """(what the golden file holds for one case, the streams): the records of the streams, or the text of the SushiError -- the
    mono file has no side mix -- with the file's path taken out."""
    from sushi_amd import SushiError
    try:
        streams = construct(how, path, top, rate, sample_type, resample)
    except SushiError as e:
        return {"error": str(e).replace(path, "<path>")}, []
    return {"streams": [record(s) for s in streams]}, streams


def key(name, sample_type, resample, how):
    return "/".join((name, sample_type, resample, how))
