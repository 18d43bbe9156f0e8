"""Mixing a WAV's channels by weight instead of averaging them.

Two releases of one programme seldom carry the same mix: a dub has its own speech over the shared bed, a 5.1 track is not the
stereo downmix of it.  Speech is centre-panned, so ``(L - R) / 2`` of a stereo file ('side') removes it from both releases and
leaves what they share; 'stereo' folds a 5.1 / 7.1 layout down the way a stereo release was made.

* ``channel_positions`` / ``weights_for`` -- named mixes as float32 weights per channel, from the file's speaker layout.
* ``mean_host`` -- the reference's channel mean of a chunk's frames (what ``'mean'`` is on the CPU path).
* ``mix_host`` -- the arithmetic of ``sushi_hip_load_decode_mix`` (include/sushi_hip.h) in NumPy, and the CPU path: bit for bit
  what the kernel writes.
* ``compare_mixes`` / ``rank_mixes`` -- which mix matches best between two releases: probes of the source searched in the whole
  destination, per mix; the ordering is a pure function of the scores.
"""
import numpy as np

from . import _native
from .common import SushiError

MAX_CHANNELS = _native.MIX_MAX_CHANNELS
MAX_OUTPUTS = _native.MIX_MAX_OUTPUTS

# dwChannelMask bits in the order their channels lie in a frame (WAVEFORMATEXTENSIBLE)
SPEAKERS = ("FL", "FR", "FC", "LFE", "BL", "BR", "FLC", "FRC", "BC", "SL", "SR", "TC", "TFL", "TFC", "TFR", "TBL", "TBC", "TBR")
# what a file without a mask holds, by channel count (the WAV default order)
DEFAULT_LAYOUTS = {1: ("FC",), 2: ("FL", "FR"), 6: ("FL", "FR", "FC", "LFE", "BL", "BR"),
                   8: ("FL", "FR", "FC", "LFE", "BL", "BR", "SL", "SR")}
NAMED_MIXES = ("side", "centre", "no_centre", "stereo")
_STEREO = {"FL": np.float32(0.5), "FR": np.float32(0.5), "FC": np.float32(0.70710678), "BL": np.float32(0.35355339),
           "BR": np.float32(0.35355339), "SL": np.float32(0.35355339), "SR": np.float32(0.35355339)}


def channel_positions(channels, mask=None):
    """Speaker names of a frame's channels, in file order: from an EXTENSIBLE fmt chunk's dwChannelMask when it names exactly
    `channels` speakers; without a mask the WAV default order for 1, 2, 6 and 8 channels; otherwise None (layout unknown)."""
    channels = int(channels)
    if mask is None:
        names = DEFAULT_LAYOUTS.get(channels)
        return None if names is None else list(names)
    mask = int(mask)
    names = [n for bit, n in enumerate(SPEAKERS) if mask >> bit & 1]
    if mask < 0 or mask >> len(SPEAKERS) or len(names) != channels:
        return None
    return names


def weights_for(mix, channels, mask=None):
    """float32[channels]: the weights of `mix` for a file of `channels` channels with speaker layout `mask` (channel_positions).
    'side': FL +0.5, FR -0.5;  'centre': FC 1;  'no_centre': 1 / k on each of the k channels that are neither FC nor LFE;
    'stereo': FL, FR 0.5, FC 0.70710678, BL, BR, SL, SR 0.35355339, LFE (and any other speaker) 0;  or an explicit sequence of
    `channels` finite numbers.  SushiError where a named mix needs speakers the layout lacks, or the layout is unknown."""
    channels = int(channels)
    if channels < 1 or channels > MAX_CHANNELS:
        raise SushiError("downmix: 1 .. %d channels, not %d" % (MAX_CHANNELS, channels))
    if not isinstance(mix, str):
        try:
            w = np.asarray(mix, dtype=np.float32).reshape(-1) if np.ndim(mix) == 1 else None
        except (TypeError, ValueError):
            w = None
        if w is None:
            raise SushiError("downmix: a mix is a name %s or a sequence of one weight per channel" % (NAMED_MIXES,))
        if w.shape[0] != channels:
            raise SushiError("downmix: %d weights for %d channels" % (w.shape[0], channels))
        if not np.isfinite(w).all():
            raise SushiError("downmix: weights must be finite")
        return w
    if mix not in NAMED_MIXES:
        raise SushiError("downmix: unknown mix %r (one of %s, 'mean', or explicit weights)" % (mix, NAMED_MIXES))
    names = channel_positions(channels, mask)
    if names is None:
        raise SushiError("downmix %r: the speaker layout of %d channels (mask %r) is unknown; give explicit weights" %
                         (mix, channels, mask))

    def need(*speakers):
        missing = [s for s in speakers if s not in names]
        if missing:
            raise SushiError("downmix %r: the layout %s has no %s" % (mix, "/".join(names), ", ".join(missing)))

    w = np.zeros(channels, np.float32)
    if mix == "side":
        need("FL", "FR")
        w[names.index("FL")], w[names.index("FR")] = 0.5, -0.5
    elif mix == "centre":
        need("FC")
        w[names.index("FC")] = 1.0
    elif mix == "no_centre":
        keep = [c for c, n in enumerate(names) if n not in ("FC", "LFE")]
        if not keep:
            raise SushiError("downmix 'no_centre': the layout %s has nothing but centre and LFE" % "/".join(names))
        w[keep] = np.float32(1.0 / len(keep))
    else:
        need("FL", "FR")
        for c, n in enumerate(names):
            w[c] = _STEREO.get(n, np.float32(0.0))
    return w


def weight_matrix(mixes, channels, mask=None):
    """float32[len(mixes), channels], C-contiguous: weights_for of every mix (1 .. 8 of them: one decode pass's rows)."""
    if not 1 <= len(mixes) <= MAX_OUTPUTS:
        raise SushiError("downmix: 1 .. %d mixes in one pass, not %d" % (MAX_OUTPUTS, len(mixes)))
    return np.ascontiguousarray(np.stack([weights_for(m, channels, mask) for m in mixes]), dtype=np.float32)


def frames_from_bytes(data, channels, sample_width):
    """int16[n, channels] of raw little-endian PCM bytes as wav.py:64-74 takes them: 16-bit samples as they are, 24-bit samples'
    top two bytes.  Bytes behind the last whole frame are dropped."""
    if sample_width not in (2, 3):
        raise SushiError('Unsupported sample width: {0}'.format(sample_width))
    raw = np.frombuffer(data, dtype=np.uint8)
    n = raw.shape[0] // (channels * sample_width)
    raw = raw[:n * channels * sample_width]
    if sample_width == 2:
        return raw.view('<i2').reshape(n, channels)
    out = np.empty(n * channels, np.int16)
    out.view(np.uint8)[0::2] = raw[1::3]
    out.view(np.uint8)[1::2] = raw[2::3]
    return out.reshape(n, channels)


def scale_float_samples(values):
    """The F32 / F64 rule of csrc/pcm_core.hpp on an array of full-scale samples (+-1.0): float32 values v become s = v * 32768.0f
    (one float32 multiply), float64 values s = float32(v * 32768.0) (a float64 multiply, one rounding, nearest-even); a NaN or
    +-inf s becomes +0.0f; denormals and -0.0 are values like any other.  Returns float32 of the same shape."""
    values = np.asarray(values)
    if values.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise SushiError('scale_float_samples: float32 or float64 samples')
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        if values.dtype == np.float32:
            s = values * np.float32(32768.0)
        else:
            s = (values * np.float64(32768.0)).astype(np.float32)
    s[~np.isfinite(s)] = np.float32(0.0)
    return s


def samples_from_bytes(data, channels, sample_format):
    """float32[n, channels] of raw little-endian frame bytes: every sample's value on the int16 scale, as csrc/pcm_core.hpp states it
    (include/sushi_hip.h "sample formats") -- the NumPy restatement of sushi_hip_load_decode_format's samples, and the CPU path.
    'u8': (b - 128) * 256;  's16' / 's24' / 's32': the top two bytes as int16 (for 's16' and 's24' frames_from_bytes as float32);
    'f32' / 'f64': scale_float_samples.  Bytes behind the last whole frame are dropped."""
    if sample_format not in _native.PCM_WIDTHS:
        raise SushiError('Unsupported sample format: {0!r}'.format(sample_format))
    width = _native.PCM_WIDTHS[sample_format]
    raw = np.frombuffer(data, dtype=np.uint8)
    n = raw.shape[0] // (channels * width)
    raw = raw[:n * channels * width]
    if sample_format == 'u8':
        return ((raw.astype(np.int32) - 128) * 256).astype(np.float32).reshape(n, channels)
    if sample_format in ('f32', 'f64'):
        values = np.frombuffer(raw.tobytes(), dtype=np.float32 if sample_format == 'f32' else np.float64)
        return scale_float_samples(values.reshape(n, channels))
    top = np.empty(n * channels, np.int16)
    top.view(np.uint8)[0::2] = raw[width - 2::width]
    top.view(np.uint8)[1::2] = raw[width - 1::width]
    return top.astype(np.float32).reshape(n, channels)


def mean_host(frames):
    """The reference's channel mean (wav.py:78-91) of int16 frames [n, C] -- or of float32 samples [n, C] (samples_from_bytes) --:
    the channels as float32 summed left to right, the sum divided by float(C) -- one channel: no division.  Returns float32[n]."""
    s = frames.astype(np.float32)
    acc = s[:, 0].copy()
    for c in range(1, s.shape[1]):
        acc += s[:, c]
    if s.shape[1] > 1:
        acc /= float(s.shape[1])
    return acc


def mix_host(frames, weights):
    """sushi_hip_load_decode_mix in NumPy, and the CPU path.  frames: int16[n, C] -- or float32 samples [n, C] (samples_from_bytes:
    sushi_hip_load_decode_mix_format) --; weights: float32[n_out, C].  Row o is
    acc = w[o][0] * s_0, then acc = acc + w[o][c] * s_c for c = 1 .. C - 1 with s_c the samples as float32: every product and
    every sum rounded to float32, every channel in file order, zero weights included.  Returns float32[n_out, n]."""
    frames = np.asarray(frames)
    w = np.asarray(weights, dtype=np.float32)
    if frames.ndim != 2 or frames.dtype not in (np.dtype(np.int16), np.dtype(np.float32)) or w.ndim != 2 or \
            w.shape[1] != frames.shape[1] or w.shape[0] < 1:
        raise SushiError("mix_host: int16 or float32 frames [n, C] and float32 weights [n_out, C]")
    s = frames.astype(np.float32)
    out = np.empty((w.shape[0], frames.shape[0]), np.float32)
    for o in range(w.shape[0]):
        acc = w[o, 0] * s[:, 0]
        for c in range(1, w.shape[1]):
            acc = acc + w[o, c] * s[:, c]
        out[o] = acc
    return out


# ---------------------------------------------------------------------------------------------- which mix is it?
def rank_mixes(names, score_matrix):
    """The decision of compare_mixes: score_matrix[k][p] is probe p's best TM_SQDIFF_NORMED score under mix names[k] (NaN: no
    such probe).  Returns [(name, median over the probes)] sorted by that median, best (lowest) first; ties keep the given order."""
    names = list(names)
    rows = [np.asarray(r, dtype=np.float64).reshape(-1) for r in score_matrix]
    if len(rows) != len(names) or not names:
        raise SushiError("rank_mixes: one row of scores per name")
    if any(r.shape[0] < 1 or np.isnan(r).all() for r in rows):
        raise SushiError("rank_mixes: every mix needs at least one probe score")
    med = [float(np.nanmedian(r)) for r in rows]
    order = np.argsort(np.asarray(med), kind="stable")
    return [(names[int(k)], med[int(k)]) for k in order]


def compare_mixes(src_streams, dst_streams, names, probes=8, probe_seconds=3.0):
    """Which of the mixes `names` matches best between two releases?  src_streams[k] / dst_streams[k]: the source and the destination
    loaded with mix names[k] (WavStream.load_mixes) -- same sample rate and type within a pair.  Per pair, `probes` slices of
    `probe_seconds` are taken from the source where estimate_speed takes them (retime.probe_starts) and searched in the whole
    destination row: one FFT-path batch of TM_SQDIFF_NORMED searches per pair.  Returns rank_mixes' list.  Needs a GPU."""
    from .device import SearchBatch
    from .retime import probe_starts
    names = list(names)
    if not (len(src_streams) == len(dst_streams) == len(names)) or not names or int(probes) < 1:
        raise SushiError("compare_mixes: one source and one destination stream per name, and probes")
    rows = []
    for name, src, dst in zip(names, src_streams, dst_streams):
        if src.sample_rate != dst.sample_rate or src.data.dtype != dst.data.dtype:
            raise SushiError("compare_mixes: source and destination must share sample rate and sample type")
        m = int(probe_seconds * src.sample_rate)
        starts = probe_starts(src.data[0], src.padding_size, src.sample_count, src.sample_rate, int(probes), m)
        if not starts:
            raise SushiError("compare_mixes: the source is flat wherever it was probed under mix %r" % (name,))
        n_dst = dst.data.shape[1]
        if m > n_dst:
            raise SushiError("compare_mixes: probes longer than the destination")
        batch = SearchBatch(dst.device_stream(), src.device_stream(), starts, [m] * len(starts), [0] * len(starts),
                            [n_dst - m + 1] * len(starts), path="fft", method="sqdiff_normed")
        batch.run()
        _, score = batch.results()
        rows.append(np.asarray(score, np.float64))
    return rank_mixes(names, rows)
