"""Drop-in for the reference's ``wav`` module (``from wav import WavStream``, sushi.py:19).

Same constructor, attributes and methods as reference wav.py:104-188; ``find_substream`` runs on
the GPU (libsushi_hip.so) instead of ``cv2.matchTemplate`` + ``argmin`` (wav.py:185-186).
Extensions: ``WavStream.from_samples`` (in-memory PCM), ``find_substreams`` (batched), ``downmix=`` / ``WavStream.load_mixes`` /
``WavStream.from_channels`` (the channels mixed by weight instead of averaged: sushi_amd/downmix.py), ``find_joint`` /
``find_joint_many`` (the one shift a group of patterns shares: sushi_amd/joint.py), ``formats='all'`` (float, 32-bit, 8-bit and
RF64 / BW64 files: the header walk below, the sample rule in sushi_amd/downmix.py ``samples_from_bytes`` / csrc/pcm_core.hpp),
``retimed`` (the stream on another clock: sushi_amd/retime.py), ``envelope`` (its loudness contour: sushi_amd/envelope.py),
``filtered`` (a band taken out of it: sushi_amd/filter.py).

The load pipeline (wav.py:64-162): the RIFF header walk on the host; PCM decode, channel downmix, decimation,
padding, the two medians, clip / scale / quantise on the GPU when one is present (the file is uploaded in bounded
chunks; sushi_amd/load.py, csrc/sushi_load.hip) and otherwise in NumPy, chunk by chunk (``_build_host``,
bit-identical; it is what the CPU tests compare with the reference-generated goldens).
``SUSHI_HIP_LOAD=host`` forces the NumPy pipeline.

How a stream comes into being: every file is read by ``_load_mixes`` (one pass, one row of frames per mix), every row of frames
becomes a stream's row in ``_build`` (the GPU or ``_build_host``; the numbers of the row's layout are ``row.row_layout``'s on both),
and every finished row is taken over by ``_adopt``, which alone makes an instance a live stream.

How one is derived from another: ``retimed``, ``envelope``, ``filtered`` and ``levelled`` each state the new stream's layout and the call that
writes its body, and ``_derive`` does the rest -- the refusal of a stream without a body, the GPU or NumPy, the row the GPU reads
(``_device_row``), the new row, its pads, its host copy, ``_adopt``.
"""
import logging
import os
import struct
import weakref
from collections import namedtuple
from time import time

import numpy as np

from .common import SushiError, clip
from .row import fill_pads, row_layout

WAVE_FORMAT_PCM = 0x0001
WAVE_FORMAT_IEEE_FLOAT = 0x0003
WAVE_FORMAT_EXTENSIBLE = 0xFFFE
# what follows the two format bytes in every SubFormat GUID that stands for a format tag (KSDATAFORMAT_SUBTYPE_*)
_SUBFORMAT_TAIL = bytes.fromhex("000000001000800000aa00389b71")
FORMATS = ('reference', 'all')


def check_formats(formats):
    if not isinstance(formats, str) or formats not in FORMATS:
        raise SushiError("Unknown formats setting of WAV stream, must be 'reference' or 'all'")


# what WavStream._requests returns
_Requests = namedtuple("_Requests", "dst_dev src_dev offs lens one_owner start_times win_start n_pos")


class DownmixedWavFile(object):
    """RIFF/WAVE reader with channel-mean downmix to float32 (reference wav.py:15-101).
    channel_mask: the dwChannelMask of an EXTENSIBLE fmt chunk that is long enough to hold one (an int), else None."""
    _file = None
    channel_mask = None
    sample_format = None    # 'u8', 's16', 's24', 's32', 'f32', 'f64'; None: a width only formats='all' decodes, read as 'reference'
    formats = 'reference'

    def __init__(self, path, formats='reference'):
        """formats: 'reference' (the default) -- the reference's parser and its refusals: RIFF, format tag 1 or 0xFFFE, 16 or 24
        bits --, or 'all': also 8-bit and 32-bit integer, 32- and 64-bit float (format tag 3, and EXTENSIBLE headers by their
        SubFormat), inside RIFF, RF64 or BW64."""
        super(DownmixedWavFile, self).__init__()
        check_formats(formats)
        self.formats = formats
        self._file = open(path, 'rb')
        try:
            head = self._file.read(12)
            rf64 = formats == 'all' and head[0:4] in (b'RF64', b'BW64')
            if head[0:4] != b'RIFF' and not rf64:
                raise SushiError('File does not start with RIFF id')
            if head[8:12] != b'WAVE':
                raise SushiError('Not a WAVE file')
            fmt_chunk_read = False
            data_chunk_read = False
            ds64_data_size = None
            file_size = os.path.getsize(path)
            while True:
                hdr = self._file.read(8)
                if len(hdr) < 8:
                    break
                name, size = hdr[0:4], struct.unpack('<L', hdr[4:8])[0]
                if formats == 'all' and name != b'data' and size == 0xFFFFFFFF:
                    raise SushiError('Invalid WAV file')              # only the data chunk's size may stand in ds64
                if rf64 and name == b'ds64':
                    # riffSize, dataSize, sampleCount (u64 each), then a table of other chunks' sizes, which is ignored
                    body = self._file.read(size + (size & 1))
                    if size < 24 or len(body) < 24:
                        raise SushiError('Invalid WAV file')
                    ds64_data_size = struct.unpack('<Q', body[8:16])[0]
                elif name == b'fmt ':
                    body = self._file.read(size + (size & 1))
                    self._read_fmt_chunk(body)
                    fmt_chunk_read = True
                elif name == b'data':
                    if not fmt_chunk_read:
                        raise SushiError('Invalid WAV file')
                    if rf64 and ds64_data_size is None:
                        raise SushiError('Invalid WAV file')          # RF64 / BW64: ds64 comes before data
                    self._data_start = self._file.tell()
                    if rf64:
                        self.frames_count = (ds64_data_size if size == 0xFFFFFFFF else size) // self.frame_size
                    elif file_size > 0xFFFFFFFF:
                        # large broken wav
                        self.frames_count = (file_size - self._file.tell()) // self.frame_size
                    else:
                        self.frames_count = size // self.frame_size
                    # what the file really holds: a data size that overstates the file (a truncated file, a
                    # 0xFFFFFFFF placeholder from a piped encoder) must not size any buffer of raw frames
                    self.frames_available = max(0, min(self.frames_count,
                                                       (file_size - self._data_start) // self.frame_size))
                    data_chunk_read = True
                    break
                else:
                    self._file.seek(size + (size & 1), 1)
            if not fmt_chunk_read or not data_chunk_read:
                raise SushiError('Invalid WAV file')
        except Exception:
            self.close()
            raise

    def __del__(self):
        self.close()

    def close(self):
        if self._file:
            self._file.close()
            self._file = None

    def _read_fmt_chunk(self, body):
        wFormatTag, self.channels_count, self.framerate, _avg, _align = struct.unpack('<HHLLH', body[:14])
        if self.formats == 'all':
            bits_per_sample = struct.unpack('<H', body[14:16])[0]
            self.sample_format = self._classify(wFormatTag, bits_per_sample, body)
            self.sample_width = (bits_per_sample + 7) // 8
        elif wFormatTag == WAVE_FORMAT_PCM or wFormatTag == WAVE_FORMAT_EXTENSIBLE:  # ignore the rest
            bits_per_sample = struct.unpack('<H', body[14:16])[0]
            self.sample_width = (bits_per_sample + 7) // 8
            self.sample_format = {2: 's16', 3: 's24'}.get(self.sample_width)      # (any other width is refused where it is decoded)
        else:
            raise SushiError('unknown format: {0}'.format(wFormatTag))
        self.frame_size = self.channels_count * self.sample_width
        if wFormatTag == WAVE_FORMAT_EXTENSIBLE and len(body) >= 24:      # cbSize, wValidBitsPerSample, then the mask
            self.channel_mask = struct.unpack('<L', body[20:24])[0]

    @staticmethod
    def _classify(tag, bits, body):
        """formats='all': the sample format of a fmt chunk.  Tag 1 by its bits (8: 'u8', 9-16: 's16', 17-24: 's24', 25-32: 's32'),
        tag 3 'f32' / 'f64'; tag 0xFFFE with a body that holds a SubFormat by the GUID's first two bytes (its fixed tail must match),
        a shorter one as PCM.  Anything else is refused by tag and bits."""
        kind = tag
        if tag == WAVE_FORMAT_EXTENSIBLE:
            kind = WAVE_FORMAT_PCM
            if len(body) >= 40:
                kind = struct.unpack('<H', body[24:26])[0] if body[26:40] == _SUBFORMAT_TAIL else None
        if kind == WAVE_FORMAT_PCM and 8 <= bits <= 32:
            return ('u8', 's16', 's24', 's32')[(bits + 7) // 8 - 1]
        if kind == WAVE_FORMAT_IEEE_FLOAT and bits in (32, 64):
            return 'f32' if bits == 32 else 'f64'
        if tag == WAVE_FORMAT_EXTENSIBLE and len(body) >= 40:
            raise SushiError('Unsupported sample format: tag 0x{0:04X}, SubFormat {1}, {2} bits'.format(tag, body[24:40].hex(), bits))
        raise SushiError('Unsupported sample format: tag 0x{0:04X}, {1} bits'.format(tag, bits))

    def frames(self, data):
        """Raw frame bytes as what the mean and the mixes work on: int16 [n, channels] for 16- and 24-bit files (frames_int16),
        float32 samples [n, channels] for the formats only formats='all' reads (sushi_amd.downmix.samples_from_bytes)."""
        if self.sample_format in (None, 's16', 's24'):
            return self.frames_int16(data)
        from .downmix import samples_from_bytes
        return samples_from_bytes(data, self.channels_count, self.sample_format)

    def frames_int16(self, data):
        """Raw frame bytes as int16 [n, channels]: what _decode averages, before it does (24-bit samples: their top two bytes)."""
        from .downmix import frames_from_bytes
        return frames_from_bytes(data, self.channels_count, self.sample_width)

    def read_raw(self, count):
        """The raw bytes of the next `count` frames (fewer at the end of the file)."""
        return self._file.read(count * self.frame_size) if count else b''

    def _decode(self, data):
        from .downmix import mean_host
        frames = self.frames(data)
        if (len(data) // self.sample_width) % self.channels_count:
            logging.error("Length of audio channels didn't match. This might result in broken output")
        return mean_host(frames)

    def readframes(self, count):
        if not count:
            return np.empty(0, np.float32)
        return self._decode(self._file.read(count * self.frame_size))

    def read_bytes_into(self, view):
        """Fill `view` (a writable bytes-like object) with the next raw frame bytes; returns how many were read."""
        return self._file.readinto(view)


_live_streams = weakref.WeakSet()


def torch_device(device):
    import torch
    d = torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if d.type == "cuda" and d.index is None else d


def _check_args(sample_type, resample, formats='reference'):
    """What every way of building a stream checks before anything else."""
    if sample_type not in ('float32', 'uint8'):
        raise SushiError('Unknown sample type of WAV stream, must be uint8 or float32')
    from .resample import check_mode
    check_mode(resample)
    check_formats(formats)


def _is_mean(downmix):
    return isinstance(downmix, str) and downmix == 'mean'


def _locate(pattern):
    """If `pattern` is a view into a live WavStream's host data (what get_substream and np.split
    of it return, sushi.py:417,445), return (stream, offset, length); else None."""
    if not isinstance(pattern, np.ndarray) or pattern.ndim != 2 or pattern.shape[0] != 1:
        return None
    if pattern.strides[1] != pattern.itemsize:
        return None
    addr = pattern.__array_interface__['data'][0]
    for s in _live_streams:
        base = s.data.__array_interface__['data'][0]
        if s.data.dtype == pattern.dtype and base <= addr and \
                addr + pattern.shape[1] * pattern.itemsize <= base + s.data.nbytes:
            return s, (addr - base) // pattern.itemsize, pattern.shape[1]
    return None


class WavStream(object):
    READ_CHUNK_SIZE = 1  # one second, seems to be the fastest
    PADDING_SECONDS = 10

    def __init__(self, path, sample_rate=12000, sample_type='uint8', device=None, downmix='mean', resample='nearest',
                 formats='reference'):
        """resample: 'nearest' (the reference's decimation, wav.py:125-137: the nearest frame, no filter) or 'fir': a zero-phase
        windowed-sinc low-pass at the file's rate in front of the decimator (sushi_amd.resample) -- on the GPU when there is one
        (sushi_hip_load_resample_fir), in NumPy otherwise, bit for bit the same; shape, time axis and everything after it unchanged.
        downmix: 'mean' (the reference's channel average, wav.py:80-91), a named mix or one weight per channel
        (sushi_amd.downmix.weights_for): the channels are then mixed by weight in the decode -- on the GPU when there is one
        (sushi_hip_load_decode_mix), in NumPy otherwise, bit for bit the same -- and everything after it is unchanged.
        formats: 'reference' (the reference's front door: RIFF, 16- or 24-bit PCM, its refusals and their text) or 'all': 8-bit and
        32-bit integer, 32- and 64-bit float files too, inside RIFF, RF64 or BW64 (DownmixedWavFile).  A sample
        becomes a float32 on the int16 scale (sushi_amd.downmix.samples_from_bytes; on the GPU sushi_hip_load_decode_format /
        _decode_mix_format, bit for bit the same), and everything after the decode -- downmix=, resample=, the clip -- is unchanged."""
        _check_args(sample_type, resample, formats)
        self._load_mixes(path, [downmix], sample_rate, sample_type, device, resample, first=self, formats=formats)

    @classmethod
    def from_samples(cls, samples, framerate, sample_rate=12000, sample_type='uint8', device=None, resample='nearest'):
        """Build a stream from downmixed PCM samples already in memory (any real dtype; values as
        DownmixedWavFile would return them), running the same pipeline as the constructor."""
        _check_args(sample_type, resample)
        self = cls.__new__(cls)
        samples = np.asarray(samples).astype(np.float32).reshape(-1)
        self._build(samples, int(framerate), samples.shape[0], sample_rate, sample_type, resample, device)
        return self

    @classmethod
    def load_mixes(cls, path, mixes, sample_rate=12000, sample_type='uint8', device=None, resample='nearest', formats='reference'):
        """[WavStream(path, downmix=m, resample=resample) for m in mixes] -- live streams, bit for bit those -- with the file read once: each chunk is
        uploaded once and one decode launch per chunk serves every weighted mix ('mean' in the list: the existing decode on the same
        uploaded chunk).  At most 8 weighted mixes.  Memory: one float32 row at the FILE's frame rate per mix (in HBM on the GPU path)
        until the last of them has been decimated.  formats: the constructor's."""
        _check_args(sample_type, resample, formats)
        mixes = list(mixes)
        if not mixes:
            raise SushiError('load_mixes: at least one mix')
        return cls._load_mixes(path, mixes, sample_rate, sample_type, device, resample, formats=formats)

    @classmethod
    def _load_mixes(cls, path, mixes, sample_rate, sample_type, device, resample, first=None, formats='reference'):
        """One stream per mix from one pass over the file -- the one place a file is read; `first`: the instance to fill for
        mixes[0] (the constructor's).  resample: every mix row is decimated on its own, so 'fir' filters each separately."""
        from .downmix import mix_host, weight_matrix
        before_read = time()
        stream = DownmixedWavFile(path, formats)
        streams = [first if (k == 0 and first is not None) else cls.__new__(cls) for k in range(len(mixes))]
        try:
            weighted = [k for k, m in enumerate(mixes) if not _is_mean(m)]
            with_mean = len(weighted) < len(mixes)
            W = weight_matrix([mixes[k] for k in weighted], stream.channels_count, stream.channel_mask) if weighted else None
            if cls._use_gpu():
                # decode + downmix on the GPU, the file uploaded in bounded chunks (sushi_amd/load.py)
                from .load import decode_file_on_device
                mono, rows, got = decode_file_on_device(stream, torch_device("cuda" if device is None else device), weights=W,
                                                        with_mean=with_mean)
            else:
                # the NumPy path: the same single pass, ten seconds of frames at a time, into one row per mix
                n = stream.frames_available
                mono = np.zeros(n, np.float32) if with_mean else None
                rows = np.zeros((len(weighted), n), np.float32) if weighted else None
                got = 0
                while got < n:
                    data = stream.read_raw(min(10 * stream.framerate, n - got))
                    m = len(data) // stream.frame_size
                    if m == 0:
                        break
                    data = data[:m * stream.frame_size]
                    if with_mean:
                        mono[got:got + m] = stream._decode(data)
                    if weighted:
                        rows[:, got:got + m] = mix_host(stream.frames(data), W)
                    got += m
            if got == 0:
                raise SushiError('no audio frames in the data chunk')
            # a file shorter than its header says: the frames that exist are decimated as the reference does (a short last
            # chunk by its own length, wav.py:127-134); what the reference leaves as uninitialised memory (np.empty,
            # wav.py:119) is zero here
            for k, new in enumerate(streams):
                samples = mono if k not in weighted else rows[weighted.index(k)]
                new._build(samples[:got], stream.framerate, stream.frames_count, sample_rate, sample_type, resample, device)
        except Exception as e:
            raise SushiError('Error while loading {0}: {1}'.format(path, e))
        finally:
            stream.close()
        plain = first is not None and _is_mean(mixes[0])        # the reference's log line for what the reference loads
        logging.info('Done reading WAV {0} in {1}s'.format(path if plain else '{0} ({1} mixes)'.format(path, len(mixes)),
                                                          time() - before_read))
        return streams

    @classmethod
    def from_channels(cls, frames, framerate, downmix, sample_rate=12000, sample_type='uint8', device=None, channel_mask=None,
                      resample='nearest'):
        """Build a stream from PCM frames already in memory -- int16 [n, channels], as DownmixedWavFile.frames_int16 returns them --
        mixed by `downmix` ('mean', a named mix or weights; channel_mask: the speaker layout a named mix reads, None: the WAV default
        order), running the same pipeline as the constructor.  float32 or float64 frames [n, channels] are samples in full-scale
        units (+-1.0), taken as a float file's are under formats='all' (sushi_amd.downmix.scale_float_samples)."""
        from .downmix import mean_host, mix_host, scale_float_samples, weight_matrix
        _check_args(sample_type, resample)
        frames = np.ascontiguousarray(frames)
        if frames.ndim != 2 or frames.dtype not in (np.dtype(np.int16), np.dtype(np.float32), np.dtype(np.float64)) or \
                frames.shape[0] < 1 or frames.shape[1] < 1:
            raise SushiError('from_channels: int16 frames [n, channels]')
        if _is_mean(downmix):
            samples = mean_host(frames if frames.dtype == np.int16 else scale_float_samples(frames))
        else:
            W = weight_matrix([downmix], frames.shape[1], channel_mask)
            if cls._use_gpu():
                from .load import mix_frames_on_device
                samples = mix_frames_on_device(frames, W, torch_device("cuda" if device is None else device))[0]
            else:
                samples = mix_host(frames if frames.dtype == np.int16 else scale_float_samples(frames), W)[0]
        self = cls.__new__(cls)
        self._build(samples, int(framerate), frames.shape[0], sample_rate, sample_type, resample, device)
        return self

    @classmethod
    def from_prepared(cls, data, sample_rate, sample_count, padding_size, device=None):
        """Wrap a (1, N) row that already is what wav.py:113-156 produces (e.g. a saved ``WavStream.data``)."""
        data = np.ascontiguousarray(data)
        if data.ndim != 2 or data.shape[0] != 1 or data.dtype not in (np.dtype(np.uint8), np.dtype(np.float32)):
            raise SushiError('Unknown sample type of WAV stream, must be uint8 or float32')
        self = cls.__new__(cls)
        self._adopt(data, None, sample_rate, sample_count, padding_size, device)
        return self

    @staticmethod
    def _use_gpu():
        """The load pipeline runs on the GPU when there is one (SUSHI_HIP_LOAD=host forces NumPy: it is what the CPU
        tests compare with the reference-generated goldens, and what bench.py uses before it forks)."""
        if os.environ.get("SUSHI_HIP_LOAD", "auto") == "host":
            return False
        try:
            import torch
            return torch.cuda.is_available()
        except ImportError:
            return False

    def _adopt(self, data, dev_row, sample_rate, sample_count, padding_size, device):
        """Become a live stream around a finished row -- every way of making a stream ends here.  data: the (1, N) host row;
        dev_row: the same row as a CUDA tensor where the GPU built it (device_stream hands it on without an upload), else None;
        device: where the matching is to run (None: the current device)."""
        self.data, self._dev_row = data, dev_row
        self.sample_rate, self.sample_count, self.padding_size = sample_rate, sample_count, padding_size
        self._device, self._dev = device, None
        _live_streams.add(self)

    def _build(self, samples, framerate, frames_count, sample_rate, sample_type, resample='nearest', device=None):
        """wav.py:113-156 on downmixed frames, a float32 host array or a float32 CUDA tensor: on the GPU if there is one -- a
        tensor always, on its own device -- (the normalised row then stays in HBM for the matching), else in NumPy."""
        if isinstance(samples, np.ndarray) and not self._use_gpu():
            return self._build_host(samples, framerate, frames_count, sample_rate, sample_type, resample, device)
        from .load import build_on_device
        data, dev_row, sample_count, padding_size = build_on_device(
            samples, framerate, frames_count, sample_rate, sample_type,
            read_chunk_size=self.READ_CHUNK_SIZE, padding_seconds=self.PADDING_SECONDS, resample=resample)
        self._adopt(data, dev_row, sample_rate, sample_count, padding_size, device)

    # wav.py:113-156 (value pipeline) in NumPy, whole-stream instead of chunk-by-chunk
    def _build_host(self, samples, framerate, frames_count, sample_rate, sample_type, resample='nearest', device=None):
        _check_args(sample_type, resample)
        lay = row_layout(samples.shape[0], framerate, frames_count, sample_rate, self.READ_CHUNK_SIZE, self.PADDING_SECONDS)
        data = np.zeros((1, lay.total), np.float32)
        pos = lay.padding_size
        if lay.downsample_rate == 1:
            data[0, pos:pos + samples.shape[0]] = samples
        elif resample == 'fir':
            # the nearest path's body length, filled by the filter instead (sushi_amd/resample.py): same layout, same time axis
            from .resample import resample_host
            if lay.n_body > lay.total - 2 * lay.padding_size:
                raise SushiError('decimated stream does not fit its buffer')
            data[0, pos:pos + lay.n_body] = resample_host(np.ascontiguousarray(samples, dtype=np.float32), framerate, sample_rate,
                                                          lay.n_body)
        else:
            # cv2.resize(..., INTER_NEAREST) per one-second chunk (wav.py:125-137):
            # x_ofs[x] = min(floor(x * (1 / (new_len / len))), len - 1)
            for length, count, start, new_length, scale_x in ((lay.chunk, lay.n_full, 0, lay.nl_full, lay.scale_full),
                                                              (lay.rest, 1, lay.n_full * lay.chunk, lay.nl_rest, lay.scale_rest)):
                if count == 0 or new_length == 0:
                    continue
                sx = np.minimum(np.floor(np.arange(new_length, dtype=np.float64) * scale_x).astype(np.int64),
                                length - 1)
                block = samples[start:start + count * length].reshape(count, length)[:, sx]
                data[0, pos:pos + count * new_length] = block.reshape(-1)
                pos += count * new_length
        # padding the audio from both sides
        fill_pads(data[0], lay.padding_size)
        # normalizing; also clipping the stream by 3*median value from both sides of zero
        max_value = float(np.median(data[data >= 0])) * 3
        min_value = float(np.median(data[data <= 0])) * 3
        np.clip(data, min_value, max_value, out=data)
        data -= min_value
        data /= (max_value - min_value)
        if sample_type == 'uint8':
            data *= 255.0
            data += 0.5
            data = data.astype('uint8')
        self._adopt(data, None, sample_rate, lay.sample_count, lay.padding_size, device)

    # ------------------------------------------------------------------ reference API
    @property
    def duration_seconds(self):
        return self.sample_count / self.sample_rate

    def get_substream(self, start, end):
        start_off = self._get_sample_for_time(start)
        end_off = self._get_sample_for_time(end)
        return self.data[:, start_off:end_off]

    def _get_sample_for_time(self, timestamp):
        # this function gets REAL sample for time, taking padding into account
        return int(self.sample_rate * timestamp) + self.padding_size

    def find_substream(self, pattern, window_center, window_size):
        diffs, times = self.find_substreams([pattern], [window_center], [window_size])
        return diffs[0], times[0]

    # ------------------------------------------------------------------ batched form
    def device_stream(self):
        """The HBM mirror of self.data (created on first use)."""
        if self._dev is None:
            from .device import DeviceStream
            row = self._dev_row
            if row is not None and (self._device is None or str(row.device) == str(torch_device(self._device))):
                self._dev = DeviceStream(row)           # already in HBM (GPU load pipeline): no H2D
            else:
                self._dev = DeviceStream(self.data[0], device=self._device)
            self._dev_row = None
        return self._dev

    def _window(self, pattern_len, window_center, window_size):
        """wav.py:178-184 -> (start_time, first sample of search_source, result length P)."""
        start_time = clip(window_center - window_size, -self.PADDING_SECONDS, self.duration_seconds)
        end_time = clip(window_center + window_size, 0, self.duration_seconds + self.PADDING_SECONDS)
        start_sample = self._get_sample_for_time(start_time)
        end_sample = self._get_sample_for_time(end_time) + pattern_len
        lo, hi, _ = slice(start_sample, end_sample).indices(self.data.shape[1])   # NumPy slice truncation
        return start_time, lo, max(hi - lo, 0) - pattern_len + 1

    def find_substreams(self, patterns, window_centers, window_sizes, with_index=False, method="sqdiff_normed"):
        """[find_substream(p, c, w) for p, c, w in zip(...)] in one GPU launch.
        Returns (diffs: float32 ndarray, times: list of float); with_index=True appends the absolute
        sample index of every match in self.data (what SpeculativeStream caches).
        method: 'sqdiff_normed' = what the reference's find_substream computes (wav.py:185-186: TM_SQDIFF_NORMED, argmin);
        'ccoeff_normed' = cv2.TM_CCOEFF_NORMED with argmax instead (not used by the reference; the method BASELINE.json names)."""
        from .device import SearchBatch
        n = len(patterns)
        r = self._requests('find_substreams', patterns, window_centers, window_sizes)
        dst_dev, src_dev = r.dst_dev, r.src_dev
        # A drop-in call is a batch of one (a triple of three): its cost is host work and launches, not arithmetic.  Such batches
        # are kept per (source stream, size, method) and RE-PLANNED in place for the next call (sushi_hip_batch_reset: no
        # allocation, one upload) instead of being built and torn down every time.
        batch = None
        pooled = n <= 4 and r.one_owner
        if pooled:
            pool = self.__dict__.setdefault("_small_batches", {})
            from .device import default_path
            key = (id(src_dev), n, method, default_path(), os.environ.get("SUSHI_HIP_EXCLUSION"))   # (what a new batch would read from the environment)
            batch = pool.get(key)
            if batch is not None and (batch.dst is not dst_dev or batch.src is not src_dev or not batch.reset(r.offs, r.lens, r.win_start, r.n_pos)):
                batch = None
        if batch is None:
            batch = SearchBatch(dst_dev, src_dev, r.offs, r.lens, r.win_start, r.n_pos, method=method, headroom=4.0 if pooled else 1.0)
            if pooled:
                pool[key] = batch
        batch.run()
        idx, score = batch.results()
        times = [st + (int(k) / float(self.sample_rate)) for st, k in zip(r.start_times, idx)]
        if with_index:
            return score, times, [int(lo) + int(k) for lo, k in zip(r.win_start, idx)]
        return score, times

    def _requests(self, who, patterns, window_centers, window_sizes, widest=False):
        """What the batched methods (`who`: the public one's name, for the error) ask of the device for their patterns and
        windows, as a _Requests record: destination DeviceStream, source DeviceStream, offsets, lengths, whether the patterns are
        views of ONE live stream; per request: start time, first sample of search_source, result length P.  widest: None for a centre or a size
        (or for the whole list) is the widest window (_widest)."""
        n = len(patterns)
        if widest:
            window_centers = [None] * n if window_centers is None else list(window_centers)
            window_sizes = [None] * n if window_sizes is None else list(window_sizes)
        if not (len(window_centers) == len(window_sizes) == n) or n == 0:
            raise SushiError('%s: need equally many patterns, centres and sizes (>= 1)' % who)
        dst_dev = self.device_stream()
        src_dev, offs, lens, one_owner = self._pattern_source(patterns, dst_dev)
        start_times, win_start, n_pos = [], [], []
        for m, c, w in zip(lens, window_centers, window_sizes):
            if widest:
                c, w = self._widest(c, w)
            st, lo, p = self._window(m, c, w)
            start_times.append(st)
            win_start.append(lo)
            n_pos.append(p)
        return _Requests(dst_dev, src_dev, offs, lens, one_owner, start_times, win_start, n_pos)

    def _pattern_source(self, patterns, dst_dev):
        """Where a batch's patterns live: (source DeviceStream, offsets, lengths, whether they are views of ONE live stream).
        Patterns that are views of one live stream are read where they are; others are uploaded as one temporary stream."""
        from .device import DeviceStream
        located = [_locate(p) for p in patterns]
        owners = set(id(l[0]) for l in located if l is not None)
        one_owner = all(l is not None for l in located) and len(owners) == 1
        if one_owner:
            src_dev = located[0][0].device_stream()
            offs = [l[1] for l in located]
            lens = [l[2] for l in located]
        else:
            # patterns that are not views of one live stream: upload them as one temporary stream
            rows = []
            for p in patterns:
                p = np.asarray(p)
                if p.ndim != 2 or p.shape[0] != 1:
                    raise SushiError('pattern must be a (1, M) array')
                if p.dtype != self.data.dtype:
                    raise SushiError('pattern and stream sample types differ')
                rows.append(np.ascontiguousarray(p[0]))
            lens = [r.shape[0] for r in rows]
            offs = list(np.concatenate(([0], np.cumsum(lens)[:-1])))
            if sum(lens) == 0:
                raise SushiError('empty pattern')
            src_dev = DeviceStream(np.concatenate(rows), device=dst_dev.device)
        return src_dev, offs, lens, one_owner

    # ------------------------------------------------------------------ every occurrence
    def find_occurrences(self, pattern, threshold, window_center=None, window_size=None, method="ccoeff_normed",
                         min_separation=None):
        """Every position of find_substream's window (wav.py:178-184) whose score passes `threshold` -- all occurrences of the
        pattern, not only the best one: np.where(result >= threshold) on wav.py:185's row for 'ccoeff_normed' (default; the
        TM_CCOEFF_NORMED value itself), np.where(result <= threshold) for 'sqdiff_normed'.  No window: the widest _window allows
        (centre duration / 2, size duration / 2 + PADDING_SECONDS: the whole stream).  min_separation (seconds, or None): keep one
        hit per occurrence -- the best, no two kept hits closer than that (sushi_amd.occurrences.peaks).  Returns (scores float32
        ndarray, times list of float) sorted by time; a time is what find_substream returns for that position."""
        return self.find_occurrences_many([pattern], threshold, [window_center], [window_size], method=method,
                                          min_separation=min_separation)[0]

    def find_occurrences_many(self, patterns, threshold, window_centers=None, window_sizes=None, method="ccoeff_normed",
                              min_separation=None, capacity=None):
        """[find_occurrences(p, threshold, c, w) for p, c, w in zip(...)] in one threshold run (patterns located as
        find_substreams does).  window_centers / window_sizes: lists (None entries, or None for the list: the widest window)."""
        from .device import SearchBatch
        from .occurrences import peaks
        r = self._requests('find_occurrences_many', patterns, window_centers, window_sizes, widest=True)
        batch = SearchBatch(r.dst_dev, r.src_dev, r.offs, r.lens, r.win_start, r.n_pos, path="fft", method=method)
        found = batch.occurrences(threshold, capacity)
        out = []
        for st, (idx, score) in zip(r.start_times, found):
            if min_separation is not None:
                idx, score = peaks(idx, score, int(round(float(min_separation) * self.sample_rate)), method)
            out.append((np.asarray(score, np.float32), [st + (int(k) / float(self.sample_rate)) for k in idx]))
        return out

    def find_best_matches(self, pattern, k, window_center=None, window_size=None, method="ccoeff_normed", min_separation=None,
                          threshold=None):
        """The k best distinct matches of the pattern in find_substream's window (wav.py:178-184), best first: is the best match
        the only one, and if not, where are the others?  Greedy suppression over wav.py:185's row (sushi_amd.occurrences.best_peaks)
        without forming it.  No window: the widest _window allows, as find_occurrences.  min_separation (seconds, or None: the
        pattern's own length -- occurrences that do not overlap); threshold: only positions that pass it.  Returns (scores float32
        ndarray, times list of float) in pick order; a time is what find_substream returns for that position.
        A k beyond the number of real occurrences is expensive without a threshold (SearchBatch.run_best)."""
        return self.find_best_matches_many([pattern], k, [window_center], [window_size], method=method,
                                           min_separation=min_separation, threshold=threshold)[0]

    def find_best_matches_many(self, patterns, k, window_centers=None, window_sizes=None, method="ccoeff_normed",
                               min_separation=None, threshold=None):
        """[find_best_matches(p, k, c, w) for p, c, w in zip(...)] in one best-k run (patterns located as find_substreams does).
        window_centers / window_sizes: lists (None entries, or None for the list: the widest window)."""
        from .device import SearchBatch
        r = self._requests('find_best_matches_many', patterns, window_centers, window_sizes, widest=True)
        batch = SearchBatch(r.dst_dev, r.src_dev, r.offs, r.lens, r.win_start, r.n_pos, path="fft", method=method)
        sep = None if min_separation is None else max(1, int(round(float(min_separation) * self.sample_rate)))
        found = batch.best(k, sep, threshold)
        return [(np.asarray(score, np.float32), [st + (int(i) / float(self.sample_rate)) for i in idx])
                for st, (idx, score) in zip(r.start_times, found)]

    def _widest(self, window_center, window_size):
        """find_occurrences' default window: the widest _window allows -- the whole stream, padding included."""
        if window_center is None:
            window_center = self.duration_seconds / 2.0
        if window_size is None:
            window_size = self.duration_seconds / 2.0 + self.PADDING_SECONDS
        return window_center, window_size

    # ------------------------------------------------------------------ whole curves
    def match_template(self, pattern, window_center, window_size, method="sqdiff_normed"):
        """wav.py:185's `result` itself: cv2.matchTemplate(search_source, pattern, method) over find_substream's window
        (wav.py:178-184), as a float32 ndarray of shape (1, P).  method: 'sqdiff_normed' (what the reference calls) or
        'ccoeff_normed' (the TM_CCOEFF_NORMED value).  Every value is the one the search path computes exactly: the argmin of
        this row (argmax for 'ccoeff_normed') and its value are what find_substream returns."""
        return self.match_templates([pattern], [window_center], [window_size], method=method)[0]

    def match_templates(self, patterns, window_centers, window_sizes, method="sqdiff_normed", as_tensor=False):
        """[match_template(p, c, w) for p, c, w in zip(...)] in one GPU launch (patterns located as find_substreams does).
        as_tensor=True: a list of (1, P) float32 CUDA tensors -- views of one device buffer, no copy to the host."""
        from .curves import match_curves
        n = len(patterns)
        r = self._requests('match_templates', patterns, window_centers, window_sizes)
        curves, bounds = match_curves(r.dst_dev, r.src_dev, r.offs, r.lens, r.win_start, r.n_pos, method=method)
        if not as_tensor:
            curves = curves.cpu().numpy()
        return [curves[int(bounds[k]):int(bounds[k + 1])].reshape(1, -1) for k in range(n)]

    # ------------------------------------------------------------------ one shift for a group
    def find_joint(self, patterns, window_centers, window_size, weights='equal', method="sqdiff_normed", with_curve=False, clamp=None,
                   capacity=None):
        """The one shift a group of patterns shares (sushi_amd.joint): pattern i is looked for at
        window_centers[i] + delta for one delta, |delta| <= window_size, scored by the weighted sum of every pattern's own score row
        at that displacement.  clamp, capacity: find_joint_many's.  Returns a JointMatch (find_joint_many)."""
        return self.find_joint_many([(patterns, window_centers)], [window_size], method=method, with_curve=with_curve,
                                    weights=weights if isinstance(weights, str) else [weights], clamp=clamp, capacity=capacity)[0]

    def find_joint_many(self, groups, window_sizes, weights='equal', method="sqdiff_normed", with_curve=False, max_bytes=None,
                        clamp=None, capacity=None):
        """[find_joint(p, c, w) for (p, c), w in zip(groups, window_sizes)]: groups is a list of (patterns, window_centers).
        Patterns are located as find_substreams locates them.  Event i of a group sits at sample bases[i] + k,
        bases[i] = _get_sample_for_time(window_centers[i]), for the displacements k every event of the group can take within
        W = int(sample_rate * window_size) samples inside the row (sushi_amd.joint.joint_window; SushiError if there is none).  All
        groups of a chunk go through one match_curves call and one sushi_hip_joint_reduce call; chunks hold whole groups under
        max_bytes of curve memory (default 1 GiB; a single group above it raises SushiError).  weights: 'equal' (1 / m), 'length'
        (M_i / sum M) or one entry per group, each one of those or a sequence of numbers.  method: 'sqdiff_normed' (first minimum of
        the sum) or 'ccoeff_normed' (first maximum).  Returns a JointMatch per group: delta (seconds; event i is found at
        window_centers[i] + delta), score, index, event_scores (every event's own score at the joint shift), event_own_delta /
        event_own_scores (what a lone search of each event over the same range finds), curve (with_curve: the float32 joint row).
        clamp (default None: nothing changes): a finite number; every event's row is then CLAMPED at f = the float32 on the failing
        side of it (sushi_amd.axis.clamp_value) -- min(R, f) under 'sqdiff_normed', max(R, f) under 'ccoeff_normed' -- and formed
        from the hits of one threshold run per chunk instead of as a whole exact row (sushi_amd.axis.event_rows): a
        position that does not pass the clamp counts as f, however badly it matches.  The answer is the exact answer of the clamped
        problem.  capacity: hits kept per event before its row is formed densely instead (None: min(n_shift, max(1024, n_shift //
        16))).  The result's event_scores stay the true scores at the chosen shift, formed one position each; an event's own
        extremum (event_own_scores) equal to f at index 0 of the axis means nothing in its window passed; clamp and rows_info say
        what was done.  Clamping pays where the threshold run's pair bound can exclude most of the window at f, and costs where
        it cannot (64 events of 3 s, +-120 s windows at 12 kHz, one MI355X): at coefficient 0.5 the run evaluates
        110 of 7564 block pairs and the whole search takes a tenth (uint8) to a thirtieth (float32) of clamp=None's time; at
        coefficient 0.3 the bound excludes nothing, every pair is evaluated and the search is 0.83 - 0.90 x as fast as clamp=None;
        a clamp that most positions pass overflows every event, which is then formed densely on top of the run: 0.45 x.  Exact
        rows of short uint8 windows are cheap: there clamp=None is the faster call.
        Needs a GPU."""
        from . import joint
        return joint.find_joint_many(self, groups, window_sizes, weights=weights, method=method, with_curve=with_curve,
                                     max_bytes=joint.MAX_BYTES if max_bytes is None else int(max_bytes), clamp=clamp, capacity=capacity)

    # ------------------------------------------------------------------ where the shared shift changes
    def find_segments(self, patterns, window_centers, window_size, penalty, weights='equal', method="sqdiff_normed", max_bytes=None,
                      max_state_bytes=None, clamp=None, capacity=None):
        """A shift for every event of a sequence, and the places where it changes (sushi_amd.segments): the events
        (patterns, window_centers: in order) are put on one shift axis -- the displacements k every event can take within
        W = int(sample_rate * window_size) samples inside the row (sushi_amd.joint.joint_window over all of them), event i at
        sample _get_sample_for_time(window_centers[i]) + k -- and a shift is chosen per event that minimises the sum of the
        events' weighted scores plus `penalty` for every change of shift between consecutive events.  Exact: the minimum over all
        assignments.  penalty (required; finite, >= 0) is in units of one event's weighted score: a change of shift must buy more
        than `penalty` of summed score, and a lone outlier between two events that agree must beat 2 x penalty.  0 gives every
        event its lone answer; a huge value gives one shift for all, the arg-min of the weighted sum.  weights: 'equal' (1.0
        each -- not 1 / m: the penalty is per event), 'length' (M_i * E / sum M) or a sequence of numbers.  method: 'sqdiff_normed'
        or 'ccoeff_normed' (the scores are negated: the larger is the better).  Patterns are located as find_substreams locates
        them.  Events go through in chunks under max_bytes of curve memory (default 1 GiB), one match_curves call and one
        sushi_hip_path_forward call each, then one backtrack; the stay bits and costs of the whole sequence, E x ceil(n_shift / 64)
        x 8 + n_shift x 8 bytes, must fit max_state_bytes (default 2 GiB; SushiError names the need).  Returns a Segmentation:
        k_lo, n_shift, shifts (samples per event), deltas (seconds), segments ([(first_event, n_events, delta)]: maximal runs of
        equal shift), cost, event_scores (every event's score at its chosen shift), event_own_delta / event_own_scores (what a
        lone search of each event over the same range finds).  clamp, capacity: find_joint_many's -- the pass then runs on rows
        clamped at f and is the exact minimum of that clamped problem (the truncated cost of labelling passes).  A change of shift
        may go either way here; the same model with the events kept in order in the destination, or with a penalty per event, is
        find_track(reach=0, order=...).  Needs a GPU."""
        from . import segments
        return segments.find_segments(self, patterns, window_centers, window_size, penalty, weights=weights, method=method,
                                      max_bytes=segments.MAX_BYTES if max_bytes is None else int(max_bytes),
                                      max_state_bytes=segments.MAX_STATE_BYTES if max_state_bytes is None else int(max_state_bytes),
                                      clamp=clamp, capacity=capacity)

    # ------------------------------------------------------------------ a shift that wanders, and may jump
    def find_track(self, patterns, window_centers, window_size, penalty, max_rate=None, reach=None, step_cost=0.0, slack=1,
                   weights='equal', method="sqdiff_normed", max_bytes=None, max_state_bytes=None, margins=False, guard=None,
                   marginals=False, clamp=None, capacity=None, order=None, wide=False):
        """A shift for every event of a sequence that may move a little from event to event and jump at a cut
        (sushi_amd.track): the events (patterns, window_centers: in order) are put on one shift axis as
        find_segments puts them, and a shift is chosen per event that minimises the sum of the events' weighted scores plus, between
        consecutive events, either step_cost per sample moved (at most reach_e samples) or `penalty` for a jump to anywhere.  Exact:
        the minimum over all assignments.  Exactly one of max_rate and reach is given: max_rate, the largest drift as a ratio (1e-4
        is 100 ppm), gives reach_e = ceil(max_rate * |base_e - base_{e-1}|) + slack samples from the events' places; reach is an
        int or one int per event (event 0's is ignored).  A reach above 1024 is a SushiError that names the event and the value.
        penalty (required; finite, >= 0) is in units of one event's weighted score, as in find_segments; step_cost (default 0: any
        move within reach is free) is in the same units per sample.  With every reach 0 the result is find_segments'.  weights,
        method, the location of patterns and max_bytes are find_segments'.  The moves and costs of the whole sequence, E x n_shift
        x 2 + 2 x n_shift x 8 bytes, must fit max_state_bytes (default 2 GiB; SushiError names the need).  Returns a Track: k_lo,
        n_shift, shifts (samples per event), deltas (seconds), reach, moves (shifts[e] - shifts[e - 1]), jumps (the events entered
        by a jump), segments ([(first_event, n_events, first_delta, last_delta)]: maximal runs without a jump), cost, event_scores,
        event_own_delta / event_own_scores (what a lone search of each event over the same range finds).
        margins=True also says how firmly every event is placed: the pass keeps every row of its costs, runs the
        same recurrence from the last event down, and the Track gains guard, event_through, event_margin -- by how much the total
        rises if the event must lie more than `guard` samples from its place: this counts what its neighbours pay too, is at most 2
        x penalty plus the event's own weighted score difference, and is inf where the axis has no such shift --, event_alt_shift /
        event_alt_delta (where it would go instead; None where there is none) and, with marginals=True, marginals (a float64 CUDA
        tensor [events, n_shift]: the cost of the best whole path through every (event, shift)).  guard is an int or one int per
        event, in samples (default int(0.01 * sample_rate), the reference's ALLOWED_ERROR).  The kept costs, another E x n_shift x 8
        + 2 x n_shift x 8 bytes (and E x n_shift x 8 for marginals), count under max_state_bytes.  A sequence that goes through in
        one chunk of max_bytes keeps its curves; one in several chunks forms every chunk's curves a second time, which doubles the
        curve work.  With margins=False (the default) nothing changes and the new fields are None.  find_segments' margins are
        find_track(reach=0, margins=True).  clamp, capacity: find_joint_many's -- the pass and its margins then run on rows clamped
        at f (every forming of a chunk, the second one for margins included) and are exact for that clamped problem.
        order keeps the events in order: no cut puts an event in the destination before the end of the event in
        front of it, so a jump into event e may lower the shift by at most back_e samples (and raise it by any amount).  None (the
        default): no limit, as before; True: back_e = max(base_e - base_{e-1} - len_{e-1}, 0) from the events' places and lengths
        (sushi_amd.track.order_back; SushiError if the events are not in order); or one int per event, -1 or None for no limit
        (event 0's is ignored).  A decoy -- a repeated jingle, a better chance match elsewhere in the window -- costs a path two
        jumps, one of which goes back further than any cut can: with order= small penalties stay safe.  penalty may also be one
        number per event (event 0's is ignored): a cut is cheap at a chapter mark and dear inside a dialogue
        (sushi_amd.shifts.chapter_penalties).  Either takes the ordered pass: its state is E x n_shift x 6 + 3 x n_shift x 8 bytes
        under max_state_bytes, the Track gains back and penalties, and margins=True with it is a SushiError (not built here:
        the ordered pass's margins are find_ordered_track's).  Moves are not restricted by order.  Without order= and with one
        penalty the code path, the launches and the bits are those of before.  Measured on one MI355X (profiles/track_order/): the
        ordered forward pass takes 12.3 x the plain one at reach 0 and 2.8 x at reach 88 (64 rows x 2.88 M shifts: 14.1 ms
        against 1.1 ms, 20.2 ms against 7.2 ms -- its prefix-minimum kernel, not tuned); a whole call on 64 uint8 events at +-120 s
        1.27 x (59.9 ms against 47.1 ms), with clamp=0.5 3.7 x (17.7 ms against 4.8 ms).
        wide=True lifts the reach's bound to 32767 samples wherever step_cost is 0 (the default): one long stretch
        without an event -- at max_rate 1e-3 a gap of more than 85 s -- no longer ends the call, and the pass walks it instead of
        paying a jump.  The model, the tie rules and the bits are the same (a wide row's window minimum is formed from prefix and
        suffix minima of 1024-value tiles, in a time that does not grow with the reach); margins=, marginals=, clamp= and chunks work
        as before; a wide call's window records, 24 bytes per shift, count under max_state_bytes.  A reach above 1024 with step_cost
        > 0 is a SushiError (such a move costs more than a jump once step_cost x reach > penalty: clip the reach), and so is wide=True
        with order= or a penalty per event: the ordered pass keeps its 1024.  With wide=False (the default) nothing changes.  Needs a
        GPU."""
        from . import track
        return track.find_track(self, patterns, window_centers, window_size, penalty, max_rate=max_rate, reach=reach,
                                step_cost=step_cost, slack=slack, weights=weights, method=method,
                                max_bytes=track.MAX_BYTES if max_bytes is None else int(max_bytes),
                                max_state_bytes=track.MAX_STATE_BYTES if max_state_bytes is None else int(max_state_bytes),
                                margins=margins, guard=guard, marginals=marginals, clamp=clamp, capacity=capacity, order=order,
                                wide=wide)

    def find_ordered_track(self, patterns, window_centers, window_size, penalty, order=None, max_rate=None, reach=None, step_cost=0.0,
                           slack=1, weights='equal', method="sqdiff_normed", max_bytes=None, max_state_bytes=None, margins=False,
                           guard=None, marginals=False, clamp=None, capacity=None, wide=False):
        """find_track through the ordered pass, and how firmly it places every event.  order and
        penalty (a number, or one per event) are find_track's; with margins=False this is find_track(order=order) -- the same
        launches, the same bits, the same Track (and with order=None and one penalty the ordered pass without a limit, whose bits
        are the plain pass's).  margins=True keeps every row of the ordered forward pass, backtracks, and walks the chunks again from
        the last one down with the backward recurrence of the ordered model -- a jump out of event e reaches shift j of event e + 1
        only from shifts up to j + back_{e+1}, which the suffix minimum read at max(j - back_{e+1}, 0) states -- so the Track's
        guard, event_through, event_margin, event_alt_shift / event_alt_delta and (marginals=True) marginals are find_track's
         for the model the caller asked for: an event that can reach its alternative only by a jump no cut can make
        is as firm as its whole run.  guard: an int or one per event, in samples (default int(0.01 * sample_rate)).  The state is E
        x n_shift x 14 + 4 x n_shift x 8 bytes (and E x n_shift x 8 for marginals) under max_state_bytes; SushiError names the
        need.  One chunk of max_bytes keeps its curves; several chunks form every chunk's rows a second time (clamp= / capacity=
        work as in find_track).  wide=True is a SushiError: the ordered pass keeps its reach of 1024 (find_track's wide form is the
        plain pass's).  Needs a GPU."""
        from . import track
        return track.find_ordered_track(self, patterns, window_centers, window_size, penalty, order=order, max_rate=max_rate, reach=reach,
                                        step_cost=step_cost, slack=slack, weights=weights, method=method,
                                        max_bytes=track.MAX_BYTES if max_bytes is None else int(max_bytes),
                                        max_state_bytes=track.MAX_STATE_BYTES if max_state_bytes is None else int(max_state_bytes),
                                        margins=margins, guard=guard, marginals=marginals, clamp=clamp, capacity=capacity, wide=wide)

    def find_ordered_wide_track(self, patterns, window_centers, window_size, penalty, order=None, max_rate=None, reach=None,
                                step_cost=0.0, slack=1, weights='equal', method="sqdiff_normed", max_bytes=None, max_state_bytes=None,
                                margins=False, guard=None, marginals=False, clamp=None, capacity=None):
        """find_ordered_track across long gaps: every argument, the Track and its margins are find_ordered_track's,
        but a reach -- given, or from max_rate -- may be up to 32767 samples, and one above 1024 needs step_cost 0 (SushiError names
        the event otherwise), as find_track(wide=True)'s does.  A programme with long stretches without an event (an opening, a
        song) and with repeated jingles or chapter marks needs both: order= and a penalty per event keep a path off the decoys, and
        the wide reach lets the shift walk across the stretch instead of paying a jump.  A row of a reach up to 1024 goes through
        find_ordered_track's own kernels: with no wider reach the Track is find_ordered_track's bit for bit; with order=None and one
        penalty it is find_track(wide=True)'s.  The state is find_ordered_track's and 24 bytes per shift of window records
        (track.ordered_wide_state_bytes) under max_state_bytes.  Needs a GPU."""
        from . import track
        return track.find_ordered_wide_track(self, patterns, window_centers, window_size, penalty, order=order, max_rate=max_rate,
                                             reach=reach, step_cost=step_cost, slack=slack, weights=weights, method=method,
                                             max_bytes=track.MAX_BYTES if max_bytes is None else int(max_bytes),
                                             max_state_bytes=track.MAX_STATE_BYTES if max_state_bytes is None else int(max_state_bytes),
                                             margins=margins, guard=guard, marginals=marginals, clamp=clamp, capacity=capacity)

    # ------------------------------------------------------------------ a shift that moves along the programme
    def find_drift(self, patterns, window_centers, window_size, max_rate, resolution=1.0, weights='equal', method="sqdiff_normed",
                   with_lines=False, max_bytes=None, clamp=None, capacity=None):
        """The line of shifts a sequence of events shares when source and destination run at slightly different rates
        (sushi_amd.drift).  The events (patterns, window_centers) are put on one shift axis -- the displacements k
        every event can take within W = int(sample_rate * window_size) samples inside the row (sushi_amd.joint.joint_window over
        all of them), event i at sample pos_i + k, pos_i = _get_sample_for_time(window_centers[i]).  Candidate rates are
        sushi_amd.drift.rate_grid(max_rate, half_span, resolution) around anchor = (min pos + max pos) // 2: steps that move the
        farthest event by `resolution` samples, out to +-max_rate (seconds of shift per second of programme).  For every rate r
        and displacement k the events' exact score rows are summed by weight, event i at k + int(np.rint(r * (pos_i - anchor))),
        and the answer is the first extremum over all (rate, k), the lowest rate first: no lone decision is made.  All rows are
        resident at once, E x n_shift x 4 bytes under max_bytes (default 1 GiB; SushiError names the need): one match_curves call,
        one sushi_hip_drift_reduce call, and one sushi_hip_joint_reduce call for every event's own lone extremum.  SushiError when
        the window leaves a candidate no displacement every event can take: window_size must cover the uncertainty of the base
        shift + max_rate x half span.  weights: 'equal' (1 / E), 'length' (M_i / sum M) or a sequence of numbers.  Returns a
        DriftMatch: rate, anchor (seconds), delta (the shift at the anchor), score, index, k_lo, n_shift, event_deltas /
        event_scores (every event on the line), event_own_delta / event_own_scores (its lone search), drift_rates / drift_scores /
        drift_deltas (the profile over rate), rate_ties, lines (with_lines).  A large speed difference goes through estimate_speed
        and retimed first; this finds the residual.  clamp, capacity: find_joint_many's -- the lines are then summed over rows
        clamped at f.  Needs a GPU."""
        from . import drift
        return drift.find_drift(self, patterns, window_centers, window_size, max_rate, resolution=resolution, weights=weights,
                                method=method, with_lines=with_lines, max_bytes=drift.MAX_BYTES if max_bytes is None else int(max_bytes),
                                clamp=clamp, capacity=capacity)

    # ------------------------------------------------------------------ one stream derived from another
    def _device_row(self, dev):
        """This stream's row as a tensor on `dev`: the mirror's if it lives there, else the GPU load pipeline's row if that does,
        else an upload of self.data[0].  Neither self._dev nor self._dev_row changes."""
        if self._dev is not None and self._dev.device == dev:
            return self._dev.raw
        if self._dev_row is not None and self._dev_row.device == dev:
            return self._dev_row
        import torch
        return torch.from_numpy(self.data[0]).to(dev)

    def _derive(self, who, plan):
        """A new live stream made from this one's row -- retimed, envelope, filtered and levelled end here.  plan(padding_size, sample_count),
        called once the body is known to lie inside the row, returns (sample_rate, padding_size, sample_count, on_host, on_device)
        of the new stream and its two writers: on_host(row, new) and on_device(row, new) write the body of the new row `new`
        (2 * padding_size + sample_count samples: an array, a tensor) from this stream's `row`.  On the GPU when there is one (the
        new row stays in HBM for the matching), else in NumPy; both pads are then filled as the loader fills them."""
        pad, count, total = int(self.padding_size), int(self.sample_count), int(self.data.shape[1])
        if count < 1 or pad < 0 or pad + count > total:
            raise SushiError('%s: the stream has no body inside its row' % who)
        new_rate, new_pad, new_count, on_host, on_device = plan(pad, count)
        if self._use_gpu():
            import torch
            dev = torch_device("cuda" if self._device is None else self._device)
            row = self._device_row(dev)
            with torch.cuda.device(dev):
                dev_row = torch.empty(2 * new_pad + new_count, dtype=row.dtype, device=dev)
                on_device(row, dev_row)
                fill_pads(dev_row, new_pad)
                data = dev_row.cpu().numpy().reshape(1, -1)
        else:
            dev_row = None
            data = np.empty((1, 2 * new_pad + new_count), self.data.dtype)
            on_host(self.data[0], data[0])
            fill_pads(data[0], new_pad)
        new = self.__class__.__new__(self.__class__)
        new._adopt(data, dev_row, new_rate, new_count, new_pad, self._device)
        return new

    # ------------------------------------------------------------------ another clock
    def retimed(self, speed):
        """This stream on the clock of a destination it plays `speed` times as fast as (sushi_amd.retime: 25/24 for PAL-sped-up
        audio against a 24 fps destination): a new live WavStream whose instant t * speed is this one's instant t.  Same sample rate,
        padding and sample type; the body has floor((sample_count - 1) * speed) + 1 samples, read from this row at a step of
        1 / speed by linear interpolation (one segment from padding_size on; a read that touches the right pad sees the edge
        value), and both pads are filled as the loader fills them.  On the GPU when there is one (sushi_hip_retime; the row stays
        in HBM for the matching), else in NumPy -- bit for bit the same.  retimed(1) holds the same samples.  Patterns cut from the
        result are ordinary views: every search method and SpeculativeStream take them as they are."""
        from .retime import as_ratio, retime_device, retime_host, speed_segment
        s = as_ratio(speed)

        def plan(pad, count):
            new_count = ((count - 1) * s.numerator) // s.denominator + 1
            segment = [speed_segment(s, pad, pad, new_count)]
            return (self.sample_rate, self.padding_size, new_count,
                    lambda row, new: retime_host(row, segment, out=new), lambda row, new: retime_device(row, segment, out=new))
        return self._derive('retimed', plan)

    # ------------------------------------------------------------------ the loudness contour
    def envelope(self, hop=8, span=4):
        """This stream's loudness contour (sushi_amd.envelope): a new live WavStream at sample_rate // hop
        (SushiError unless hop divides the rate) whose sample k is the mean absolute deviation, about the sample type's nominal
        centre, of span blocks of hop samples -- twice that mean, so that a full-scale square wave gives full scale.  With
        a = (span - 1) // 2, sample k of the body covers the source instants [(k - a) * hop, (k - a + span) * hop) / sample_rate
        of this stream's body; reads outside the row see its edge samples.  Source and destination of a search are enveloped with
        the same hop and span and so get the same offset: shifts are unaffected.  padding_size // hop samples of padding, filled as
        the loader fills them, ceil(sample_count / hop) samples of body, the same sample type.  What survives is what two releases
        share when their waveforms do not: inverted polarity, a speed change with the pitch kept (envelope().retimed(speed) puts
        the contour on the destination's clock), another carrier under the same contour.  On the GPU when there is one
        (sushi_hip_envelope; the row stays in HBM for the matching), else in NumPy -- bit for bit the same.  The result is an
        ordinary stream: every search method, SpeculativeStream, retimed and estimate_speed take it as it is."""
        from .envelope import envelope_device, envelope_host, envelope_layout

        def plan(pad, count):
            new_rate, new_pad, new_count = envelope_layout(self.sample_rate, pad, count, hop)
            body = slice(new_pad, new_pad + new_count)

            def on_host(row, new):
                new[body] = envelope_host(row, pad, hop, span, new_count)
            return (new_rate, new_pad, new_count, on_host,
                    lambda row, new: envelope_device(row, pad, hop, span, new_count, out=new[body]))
        return self._derive('envelope', plan)

    # ------------------------------------------------------------------ a band removed
    def filtered(self, low=None, high=None, stop=False, n_taps=255, taps=None):
        """This stream through a FIR filter (sushi_amd.filter): a new live WavStream with the same sample rate,
        padding_size, sample_count and sample type.  The taps are filter.band_taps(sample_rate, low, high, n_taps, stop) -- only
        low: a high-pass (filtered(low=150) takes mains hum, DC wander and rumble out), only high: a low-pass, both: a band-pass,
        stop=True: what those leave -- or `taps` as given (an odd number of finite values, up to 2047; taps[k] meets the sample
        (len - 1) // 2 - k places in front of the output: filter.preemphasis_taps()).  The body is filtered about the sample type's
        nominal centre; reads past the body see the pads, reads past the row its edge samples; both pads are then filled as the
        loader fills them.  Source and destination of a search are filtered alike and so get the same delay: shifts are
        unaffected, also for taps that are not symmetric.  On the GPU when there is one (sushi_hip_filter; the row stays in HBM for
        the matching), else in NumPy -- bit for bit the same.  The result is an ordinary stream: every search method,
        SpeculativeStream, retimed and envelope take it as it is."""
        from .filter import band_taps, filter_device, filter_host

        def plan(pad, count):
            h = band_taps(self.sample_rate, low, high, n_taps, stop) if taps is None else np.asarray(taps, np.float64)
            body = slice(pad, pad + count)

            def on_host(row, new):
                new[body] = filter_host(row, pad, h, count)
            return (self.sample_rate, self.padding_size, count, on_host,
                    lambda row, new: filter_device(row, pad, h, count, out=new[body]))
        return self._derive('filtered', plan)

    # ------------------------------------------------------------------ the local level divided out
    def levelled(self, window=129, floor=1 / 128, peak=8.0):
        """This stream with every sample divided by the local level (sushi_amd.level): a new live WavStream with
        the same sample rate, padding_size, sample_count and sample type.  The local level is the mean absolute deviation, about
        the sample type's nominal centre, over `window` samples around the sample (odd, up to 1023; 129 is about 10 ms at
        12 kHz); level * peak maps to full scale and what exceeds it is clamped; `floor`, a fraction of the half range, is added
        to the level so that digital silence stays at the centre and quantisation noise is not blown up to full scale (1 / 128:
        one step of a uint8 stream).  What it is for: two mono dubs that share a music-and-effects bed under louder speech of
        their own -- a normalised score weights each instant by its energy, so the unrelated speech decides it; levelled, the
        bed in the pauses between words and syllables counts as much as the words -- and captures through an AGC or a broadcast
        compressor.  The body is levelled with reads past the body seeing the pads and reads past the row its edge samples; both
        pads are then filled as the loader fills them.  Source and destination of a search are levelled alike, so shifts are
        unaffected.  filtered(...).levelled() composes (a band removed first, then the level); levelled().envelope() is nearly
        flat by construction and therefore useless.  On the GPU when there is one (sushi_hip_level; the row stays in HBM for the
        matching), else in NumPy -- bit for bit the same.  The result is an ordinary stream: every search method,
        SpeculativeStream, retimed and filtered take it as it is."""
        from .level import _check, level_device, level_host

        def plan(pad, count):
            _check(pad + count, pad, window, floor, peak, count)
            body = slice(pad, pad + count)

            def on_host(row, new):
                new[body] = level_host(row, pad, window, floor, peak, count)
            return (self.sample_rate, self.padding_size, count, on_host,
                    lambda row, new: level_device(row, pad, window, floor, peak, count, out=new[body]))
        return self._derive('levelled', plan)
