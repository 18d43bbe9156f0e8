"""WavStream's value pipeline on the GPU (reference wav.py:113-156 after the RIFF decode).

Host: RIFF parse + channel downmix (``DownmixedWavFile``), the chunk bookkeeping of wav.py:113-137
(how many samples each one-second chunk becomes) and the 256-bin bucket walks of the radix select.
Device (libsushi_hip.so, csrc/sushi_load.hip): decimation + padding, the histograms behind the two
medians, clip / scale / quantise.  The result is bit-identical to ``wav.WavStream._build_host`` and the
normalised stream never crosses PCIe twice: the device copy is handed to ``DeviceStream`` as is.
"""
import ctypes
import logging

import numpy as np
import torch

from . import _native
from .common import SushiError
from .row import row_layout
from .wav import _check_args


def _select(L, data, n, side, rank, hist, stream):
    """Key (uint32) of the element of ascending-key rank `rank` among the samples of one side."""
    prefix, mask = 0, 0
    for shift in (24, 16, 8, 0):
        _native.check(L.sushi_hip_load_histogram(data.data_ptr(), n, side, prefix, mask, shift, hist.data_ptr(), stream),
                      "sushi_hip_load_histogram")
        h = hist.cpu().numpy()
        c = np.cumsum(h)
        b = int(np.searchsorted(c, rank, side="right"))
        if b > 255:
            raise SushiError("radix select: rank outside the population")
        rank -= int(c[b - 1]) if b else 0
        prefix |= b << shift
        mask |= 0xFF << shift
    return prefix


def _median(L, data, n, side, hist, stream):
    """np.median(data[data >= 0]) (side 0) / np.median(data[data <= 0]) (side 1) as a Python float."""
    _native.check(L.sushi_hip_load_histogram(data.data_ptr(), n, side, 0, 0, 24, hist.data_ptr(), stream),
                  "sushi_hip_load_histogram")
    m = int(hist.cpu().numpy().sum())
    if m == 0:
        raise SushiError("stream has no samples on one side of zero")

    def value(ascending_rank):
        # side 1 holds keys of -x: ascending x is descending key
        r = ascending_rank if side == 0 else m - 1 - ascending_rank
        v = np.array([_select(L, data, n, side, r, hist, stream)], np.uint32).view(np.float32)[0]
        return v if side == 0 else np.float32(-v)

    if m % 2:
        return float(value(m // 2))
    lo, hi = value(m // 2 - 1), value(m // 2)
    return float(np.float32(lo + hi) / np.float32(2.0))       # np.mean of two float32 values


UPLOAD_CHUNK_BYTES = 32 << 20      # PCM bytes uploaded and decoded per step: bounds the host memory of a load


def decode_mix_on_device(L, staged, n_frames, channels, sample_width, weights, rows, first, st, sample_format=None):
    """One sushi_hip_load_decode_mix launch: frames [0, n_frames) of the uploaded PCM bytes `staged` under the float32 weights
    [n_out, channels] (a C-contiguous host array) go to rows[o, first : first + n_frames] of the float32 CUDA tensor `rows`.
    sample_format (one of the formats _uses_format_entry names): the launch is sushi_hip_load_decode_mix_format's instead."""
    if _uses_format_entry(sample_format):
        _native.check(L.sushi_hip_load_decode_mix_format(staged.data_ptr(), n_frames, channels, _native.PCM_FORMATS[sample_format],
                                                         weights.ctypes.data, weights.shape[0], rows.data_ptr() + 4 * first,
                                                         rows.stride(0), st), "sushi_hip_load_decode_mix_format")
        return
    _native.check(L.sushi_hip_load_decode_mix(staged.data_ptr(), n_frames, channels, sample_width, weights.ctypes.data,
                                              weights.shape[0], rows.data_ptr() + 4 * first, rows.stride(0), st),
                  "sushi_hip_load_decode_mix")


def _uses_format_entry(sample_format):
    """16- and 24-bit files (and a file read without a format: 'reference') keep the existing decode entry points, launch for launch;
    'u8', 's32', 'f32' and 'f64' go through sushi_hip_load_decode_format / _decode_mix_format (csrc/sushi_pcm.hip)."""
    return sample_format not in (None, 's16', 's24')


def decode_file_on_device(wavfile, dev, weights=None, with_mean=False):
    """wav.py:64-91 on the GPU: the data chunk of `wavfile` (a DownmixedWavFile positioned at its first frame) is
    read UPLOAD_CHUNK_BYTES at a time, uploaded, decoded and downmixed by sushi_hip_load_decode into one float32
    mono tensor.  Host memory: one chunk of file bytes.  A file whose sample_format is 'u8', 's32', 'f32' or 'f64' (read with
    formats='all') takes sushi_hip_load_decode_format / _decode_mix_format instead, chunk by chunk in the same way.
    weights (float32 [n_out, channels], sushi_amd.downmix.weight_matrix): every chunk is still read and uploaded once, and one
    sushi_hip_load_decode_mix launch on it writes all n_out weighted rows; the channel mean is then decoded only with with_mean=True,
    by the existing entry on the same uploaded chunk.  Returns (mean tensor [frames] or None, rows tensor [n_out, frames] or None,
    frames).  Device memory: one float32 row at the file's frame rate per mix."""
    L = _native.lib()
    frame_size = wavfile.frame_size
    sample_format = getattr(wavfile, 'sample_format', None)
    if _uses_format_entry(sample_format):
        if sample_format not in _native.PCM_FORMATS or wavfile.sample_width != _native.PCM_WIDTHS[sample_format]:
            raise SushiError('Unsupported sample format: {0!r}'.format(sample_format))
    elif wavfile.sample_width not in (2, 3):
        raise SushiError('Unsupported sample width: {0}'.format(wavfile.sample_width))
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        if weights.ndim != 2 or weights.shape[1] != wavfile.channels_count or not 1 <= weights.shape[0] <= _native.MIX_MAX_OUTPUTS:
            raise SushiError('downmix: weights must be [1 .. %d, channels]' % _native.MIX_MAX_OUTPUTS)
    want_mean = weights is None or with_mean
    frames_total = int(wavfile.frames_available)           # never more than the file holds, whatever the header says
    frames_per_chunk = max(1, UPLOAD_CHUNK_BYTES // frame_size)
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        mono = torch.zeros(max(frames_total, 1), dtype=torch.float32, device=dev) if want_mean else None
        rows = None if weights is None else torch.zeros((weights.shape[0], max(frames_total, 1)), dtype=torch.float32, device=dev)
        stage = bytearray(min(frames_per_chunk, max(frames_total, 1)) * frame_size)     # the one host buffer of the load
        done = 0
        while done < frames_total:
            want = min(frames_per_chunk, frames_total - done)
            nbytes = wavfile.read_bytes_into(memoryview(stage)[:want * frame_size])
            got = nbytes // frame_size
            if got == 0:
                break                                            # file shorter than its header says
            if nbytes != got * frame_size:
                logging.error("Length of audio channels didn't match. This might result in broken output")
            # (a pageable-memory upload returns when the bytes have left `stage`: it can be refilled right away)
            staged = torch.frombuffer(stage, dtype=torch.uint8, count=got * frame_size).to(dev)
            if want_mean and _uses_format_entry(sample_format):
                _native.check(L.sushi_hip_load_decode_format(staged.data_ptr(), got, wavfile.channels_count,
                                                             _native.PCM_FORMATS[sample_format], mono.data_ptr() + 4 * done, st),
                              "sushi_hip_load_decode_format")
            elif want_mean:
                _native.check(L.sushi_hip_load_decode(staged.data_ptr(), got, wavfile.channels_count, wavfile.sample_width,
                                                      mono.data_ptr() + 4 * done, st), "sushi_hip_load_decode")
            if rows is not None:
                decode_mix_on_device(L, staged, got, wavfile.channels_count, wavfile.sample_width, weights, rows, done, st,
                                     sample_format)
            done += got
            del staged                                           # stream-ordered free: the kernels above are queued first
    keep = max(done, 1)                                       # the frames that were there (n_raw of the pipeline)
    return (None if mono is None else mono[:keep]), (None if rows is None else rows[:, :keep]), done


def mix_frames_on_device(frames, weights, dev):
    """mix_host on the GPU for frames already in memory: int16 frames [n, channels] (C-contiguous) under the float32 weights
    [n_out, channels] -> a float32 CUDA tensor [n_out, n] on `dev`.  One upload, one sushi_hip_load_decode_mix launch.
    float32 / float64 frames: full-scale samples, mixed as an 'f32' / 'f64' file's (one sushi_hip_load_decode_mix_format launch)."""
    n, channels = frames.shape
    sample_format = {np.dtype(np.int16): None, np.dtype(np.float32): 'f32', np.dtype(np.float64): 'f64'}[frames.dtype]
    with torch.cuda.device(dev):
        staged = torch.from_numpy(frames.reshape(-1).view(np.uint8)).to(dev)
        rows = torch.empty((weights.shape[0], n), dtype=torch.float32, device=dev)
        decode_mix_on_device(_native.lib(), staged, n, channels, 2, weights, rows, 0, torch.cuda.current_stream(dev).cuda_stream,
                             sample_format)
    return rows


def build_on_device(samples, framerate, frames_count, sample_rate, sample_type, device=None, read_chunk_size=1,
                    padding_seconds=10, resample='nearest'):
    """-> (host data ndarray (1, L) of dtype uint8/float32, device tensor of the same row, sample_count, padding_size)
    `samples`: downmixed frames, a float32 host array or a float32 CUDA tensor (decode_file_on_device).
    resample='fir': the decimation step alone is sushi_hip_load_resample_fir (sushi_amd/resample.py) -- the same layout, a low-pass
    in front of the decimator; the medians, the normalisation and the hand-over are the code below either way."""
    from .resample import resample_device
    _check_args(sample_type, resample)
    L = _native.lib()
    on_device = isinstance(samples, torch.Tensor)
    dev = samples.device if on_device else \
        (torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device))
    n_raw = int(samples.shape[0])
    lay = row_layout(n_raw, framerate, frames_count, sample_rate, read_chunk_size, padding_seconds)
    total, padding_size = lay.total, lay.padding_size
    if lay.downsample_rate != 1 and lay.nl_full <= 0:
        raise SushiError('sample rate too low for one-second chunks')
    if total - 2 * padding_size < lay.n_body:
        raise SushiError('decimated stream does not fit its buffer')         # np.copyto would raise in the reference
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        raw = samples if on_device else torch.from_numpy(np.ascontiguousarray(samples, dtype=np.float32)).to(dev)
        data = torch.empty(total, dtype=torch.float32, device=dev)
        if resample == 'fir' and lay.downsample_rate != 1:
            resample_device(raw, framerate, sample_rate, lay.n_body, padding_size, total, out=data)
        else:
            _native.check(L.sushi_hip_load_resample(raw.data_ptr(), n_raw, lay.chunk, lay.nl_full, lay.scale_full, lay.n_full,
                                                    lay.rest, lay.nl_rest, lay.scale_rest, padding_size, total, data.data_ptr(), st),
                          "sushi_hip_load_resample")
        hist = torch.empty(256, dtype=torch.int64, device=dev)
        max_value = _median(L, data, total, 0, hist, st) * 3
        min_value = _median(L, data, total, 1, hist, st) * 3
        lo, hi, rng = np.float32(min_value), np.float32(max_value), np.float32(max_value - min_value)
        u8 = torch.empty(total, dtype=torch.uint8, device=dev) if sample_type == 'uint8' else None
        _native.check(L.sushi_hip_load_normalise(data.data_ptr(), total, ctypes.c_float(lo), ctypes.c_float(hi),
                                                 ctypes.c_float(rng), u8.data_ptr() if u8 is not None else None, st),
                      "sushi_hip_load_normalise")
        row = u8 if u8 is not None else data
        host = row.cpu().numpy().reshape(1, -1)
    return host, row, lay.sample_count, padding_size
