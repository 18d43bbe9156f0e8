"""The layout of a WavStream's row (reference wav.py:113-137) and the filling of its pads (wav.py:140-141): host-only, no torch.

One place for the numbers both load paths need -- ``WavStream._build_host`` (NumPy) and ``load.build_on_device`` (the GPU) -- so
that they agree by construction.
"""
import collections
import math

from .common import py2_round

RowLayout = collections.namedtuple("RowLayout", [
    "sample_count",       # math.ceil(total_seconds * sample_rate): the body the header promises
    "padding_size",       # samples of padding on either side of it
    "total",              # the row's length
    "downsample_rate",    # sample_rate / float(framerate); 1: the frames are copied as they are
    "chunk",              # frames of one read (READ_CHUNK_SIZE seconds)
    "n_full", "rest",     # whole chunks among the n_raw frames, and the frames of the last, shorter one
    "nl_full", "nl_rest",         # samples a whole chunk and the last one become (0: the chunk is skipped)
    "scale_full", "scale_rest",   # cv2.resize's scale_x of either, 1.0 / (new_length / length); 0.0 for a skipped chunk
    "n_body",             # samples the chunks write: n_full * nl_full + nl_rest
])


def row_layout(n_raw, framerate, frames_count, sample_rate, read_chunk_size=1, padding_seconds=10):
    """The row that `n_raw` frames at `framerate` become at `sample_rate`, for a file whose header says `frames_count` frames
    (wav.py:113-120, and the lengths of wav.py:125-137's one-second chunks).  The formulas and the order of their float operations
    are the reference's.  As there, `padding_seconds` sizes the row and the pad itself is 10 seconds whatever it says.
    What the callers do with it differs in one place, kept as it is: where a whole chunk would become no sample (nl_full == 0)
    the NumPy path skips the chunk, as it skips such a last chunk, while the device path refuses the load ('sample rate too low
    for one-second chunks'); and only the device path and the NumPy path's 'fir' branch check n_body against the row before
    they write (NumPy's own assignment raises in the nearest branch)."""
    total_seconds = frames_count / float(framerate)
    downsample_rate = sample_rate / float(framerate)
    sample_count = math.ceil(total_seconds * sample_rate)
    padding_size = 10 * framerate
    total = int(padding_seconds * 2 * framerate + sample_count)
    chunk = int(read_chunk_size * framerate)
    n_full, rest = divmod(int(n_raw), chunk)
    nl_full = max(int(py2_round(chunk * downsample_rate)), 0)
    nl_rest = max(int(py2_round(rest * downsample_rate)), 0) if rest else 0
    scale_full = 1.0 / (float(nl_full) / float(chunk)) if nl_full > 0 else 0.0
    scale_rest = 1.0 / (float(nl_rest) / float(rest)) if nl_rest > 0 else 0.0
    return RowLayout(sample_count, padding_size, total, downsample_rate, chunk, n_full, rest, nl_full, nl_rest, scale_full,
                     scale_rest, n_full * nl_full + nl_rest)


def fill_pads(row, pad):
    """Both pads of a 1-D row (an ndarray or a tensor) take the value of the neighbouring inner sample, as wav.py:140-141 fills
    them.  pad == 0: nothing to fill."""
    if pad:
        row[:pad] = row[pad]
        row[-pad:] = row[-pad - 1]
