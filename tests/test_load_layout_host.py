"""sushi_amd.row.row_layout -- the one place both load paths take a row's numbers from -- against a transcription of the
reference's own loop (wav.py:113-137), chunk by chunk, and fill_pads against wav.py:140-141.  No GPU."""
import math

import numpy as np
import pytest

from sushi_amd.common import py2_round
from sushi_amd.row import RowLayout, fill_pads, row_layout

READ_CHUNK_SIZE, PADDING_SECONDS = 1, 10


def _reference_loop(n_raw, framerate, frames_count, sample_rate):
    """wav.py:113-137 with the file replaced by a count of the frames left in it: -> (sample_count, padding_size, row length,
    [(frames read, new_length, scale_x)] per pass of the loop that wrote samples, samples written).  round() is Python 2's;
    scale_x is cv2.resize's, 1.0 / (dsize.width / ssize.width), as the NumPy path states it."""
    total_seconds = frames_count / float(framerate)
    downsample_rate = sample_rate / float(framerate)
    sample_count = math.ceil(total_seconds * sample_rate)
    total = int(PADDING_SECONDS * 2 * framerate + sample_count)
    padding_size = 10 * framerate
    seconds_read, samples_read, left, passes = 0, padding_size, n_raw, []
    while seconds_read < total_seconds:
        length = min(int(READ_CHUNK_SIZE * framerate), left)          # readframes: what is there, at most a chunk
        left -= length
        new_length = int(py2_round(length * downsample_rate))
        if new_length:
            passes.append((length, new_length, 1.0 / (float(new_length) / float(length))))
        samples_read += new_length
        seconds_read += READ_CHUNK_SIZE
    assert left == 0
    return sample_count, padding_size, total, passes, samples_read - padding_size


def _frame_counts(framerate):
    chunk = READ_CHUNK_SIZE * framerate
    return [1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1234]


@pytest.mark.parametrize("overclaim", [0, 1, 30001], ids=["header-true", "header-one-more", "header-30001-more"])
@pytest.mark.parametrize("framerate,sample_rate", [(12000, 12000), (48000, 12000), (44100, 12000), (22050, 12000), (96000, 12000),
                                                   (8000, 12000)])
def test_row_layout_equals_the_reference_loop(framerate, sample_rate, overclaim):
    for n_raw in _frame_counts(framerate):
        frames_count = n_raw + overclaim
        sample_count, padding_size, total, passes, written = _reference_loop(n_raw, framerate, frames_count, sample_rate)
        chunk = READ_CHUNK_SIZE * framerate
        n_full, rest = divmod(n_raw, chunk)
        (_, nl_full, scale_full), = _reference_loop(chunk, framerate, chunk, sample_rate)[3]     # what a whole chunk becomes
        assert passes[:n_full] == [(chunk, nl_full, scale_full)] * n_full and len(passes) <= n_full + 1
        _, nl_rest, scale_rest = passes[n_full] if len(passes) > n_full else (rest, 0, 0.0)       # a last chunk that wrote nothing
        assert len(passes) == n_full or passes[n_full][0] == rest
        want = RowLayout(sample_count=sample_count, padding_size=padding_size, total=total,
                         downsample_rate=sample_rate / float(framerate), chunk=chunk, n_full=n_full, rest=rest, nl_full=nl_full,
                         nl_rest=nl_rest, scale_full=scale_full, scale_rest=scale_rest, n_body=written)
        got = row_layout(n_raw, framerate, frames_count, sample_rate, READ_CHUNK_SIZE, PADDING_SECONDS)
        where = (framerate, sample_rate, n_raw, frames_count)
        assert got == want, where
        for a, b in zip(got, want):
            assert type(a) is type(b), where                       # an int stays an int, a float a float
        assert got.n_body == got.n_full * got.nl_full + got.nl_rest == written, where
        assert got.n_body <= got.total - 2 * got.padding_size, where


def test_row_layout_hand_computed():
    # 48 -> 12 kHz, two seconds and two frames: py2_round(0.5) == 1 where Python 3's round gives 0
    lay = row_layout(96002, 48000, 96002, 12000)
    assert lay == RowLayout(24001, 480000, 984001, 0.25, 48000, 2, 2, 12000, 1, 4.0, 2.0, 24001)
    # one frame left over: it becomes no sample, the chunk is skipped
    lay = row_layout(96001, 48000, 96001, 12000)
    assert (lay.rest, lay.nl_rest, lay.scale_rest, lay.n_body, lay.sample_count) == (1, 0, 0.0, 24000, 24001)
    # the pad is ten seconds whatever padding_seconds says; the row's length follows it (wav.py:119-120)
    lay = row_layout(12000, 12000, 12000, 12000, padding_seconds=3)
    assert (lay.padding_size, lay.total, lay.downsample_rate, lay.n_body) == (120000, 84000, 1.0, 12000)
    # a sample rate at which a whole chunk becomes nothing: the callers decide what that means
    lay = row_layout(200, 100, 200, 0.001)
    assert (lay.nl_full, lay.scale_full, lay.n_body) == (0, 0.0, 0)


def test_fill_pads():
    row = np.arange(10, dtype=np.float32)
    fill_pads(row, 3)
    assert row.tolist() == [3, 3, 3, 3, 4, 5, 6, 6, 6, 6]
    row = np.arange(10, dtype=np.uint8)
    fill_pads(row, 0)                                             # nothing to fill: not the whole row
    assert row.tolist() == list(range(10))
    import torch
    t = torch.arange(10, dtype=torch.float32)
    fill_pads(t, 4)
    assert t.tolist() == [4, 4, 4, 4, 4, 5, 5, 5, 5, 5]
