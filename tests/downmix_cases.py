"""Seeded inputs of the weighted-downmix tests (TEST INFRASTRUCTURE): a WAV writer that knows EXTENSIBLE fmt chunks and 24-bit
samples, and the stereo dub of DESIGN.md 3.13 -- two releases that share a stereo bed and carry their own centre-panned speech."""
import math
import struct

import numpy as np

from sushi_amd import synth

RATE = 12000
DUB_SECONDS = 60
DUB_OFFSET = 1234                       # source sample t is destination sample t + 1234
DUB_EVENTS = (12.0, 20.0, 31.0, 44.0)   # starts of the 2 s patterns (source time); 12 s and 44 s lie under speech
DUB_WINDOW = 2000                       # samples on each side

KSDATAFORMAT_SUBTYPE_PCM = bytes.fromhex("0100000000001000800000aa00389b71")


def pcm_bytes(frames, width):
    """int [n, C] -> little-endian PCM bytes: int16 values for width 2; for width 3 the 24-bit values."""
    frames = np.asarray(frames)
    if width == 2:
        return frames.astype('<i2').tobytes()
    v = frames.astype('<i4').reshape(-1)
    return np.ascontiguousarray(v.view(np.uint8).reshape(-1, 4)[:, :3]).tobytes()


def write_wav(path, frames, rate, width=2, mask=None, claim_frames=None):
    """frames: int [n, C].  mask: None -> a plain PCM fmt chunk; an int -> WAVE_FORMAT_EXTENSIBLE with that dwChannelMask.
    claim_frames: what the data chunk's size field says (default: the truth)."""
    frames = np.asarray(frames)
    ch = frames.shape[1]
    data = pcm_bytes(frames, width)
    claimed = len(data) if claim_frames is None else claim_frames * ch * width
    if mask is None:
        fmt = struct.pack('<HHLLHH', 1, ch, rate, rate * ch * width, ch * width, 8 * width)
    else:
        fmt = struct.pack('<HHLLHHHHL', 0xFFFE, ch, rate, rate * ch * width, ch * width, 8 * width, 22, 8 * width, mask) + \
            KSDATAFORMAT_SUBTYPE_PCM
    with open(path, 'wb') as f:
        f.write(b'RIFF' + struct.pack('<L', 4 + 8 + len(fmt) + 8 + claimed) + b'WAVE')
        f.write(b'fmt ' + struct.pack('<L', len(fmt)) + fmt)
        f.write(b'data' + struct.pack('<L', claimed))
        f.write(data)


def random_frames(n, channels, width, seed):
    """Seeded frames [n, C] over the whole range of the sample width."""
    rng = np.random.default_rng(seed)
    lim = 1 << (8 * width - 1)
    return rng.integers(-lim, lim, (n, channels), dtype=np.int64)


def mix_weights(n_out, channels, seed):
    """Seeded weights with what an arithmetic can get wrong in them: zeros of both signs, +-1, values that are not dyadic."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((n_out, channels)).astype(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 0.70710678, 1.0 / 3.0], np.float32)
    pick = rng.random((n_out, channels)) < 0.3
    w[pick] = special[rng.integers(0, special.shape[0], int(pick.sum()))]
    return np.ascontiguousarray(w)


def dub_frames():
    """(destination int16 [n, 2], source int16 [n, 2], gate bool[n]): beds make_dst_pcm seeds 1 (L) and 2 (R) x 0.35; speech seeds 3
    (destination) and 4 (source) x 0.6 where speech_gate(n, rate, 5) is on, the same in L and R; the source is bed and speech
    advanced by DUB_OFFSET plus white noise 30 dB under the L bed on each channel (default_rng(9), L first)."""
    n = DUB_SECONDS * RATE
    bed = [synth.make_dst_pcm(DUB_SECONDS, RATE, seed=s).astype(np.float64) * 0.35 for s in (1, 2)]
    gate = synth.speech_gate(n, RATE, 5)
    sp_dst = synth.make_dst_pcm(DUB_SECONDS, RATE, seed=3).astype(np.float64) * 0.6 * gate
    sp_src = synth.make_dst_pcm(DUB_SECONDS, RATE, seed=4).astype(np.float64) * 0.6 * gate
    rng = np.random.default_rng(9)
    sigma = math.sqrt(float(np.mean(bed[0] ** 2)) / 1000.0)
    to16 = lambda v: np.clip(np.round(v), -32768, 32767).astype(np.int16)
    dst = np.stack([to16(b + sp_dst) for b in bed], axis=1)
    src = np.stack([to16(synth._shifted(b, DUB_OFFSET) + synth._shifted(sp_src, DUB_OFFSET) + rng.standard_normal(n) * sigma)
                    for b in bed], axis=1)
    return dst, src, gate
