"""WavStream.retimed / envelope / filtered come from one derive path (sushi_amd/wav.py _derive): the refusal of a stream without a
body, and what every derived stream is -- adopted, live, laid out as its method says, padded as the loader pads.  Host path."""
from fractions import Fraction

import numpy as np
import pytest

from sushi_amd import synth
from sushi_amd.common import SushiError
from sushi_amd.wav import WavStream, _locate

RATE = 2000
SPEED = Fraction(25, 24)
METHODS = {
    "retimed": lambda w: w.retimed(1),
    "envelope": lambda w: w.envelope(8, 4),
    "filtered": lambda w: w.filtered(low=150),
}


@pytest.mark.parametrize("name", sorted(METHODS))
@pytest.mark.parametrize("count,pad", [(0, 8), (40, 30), (40, -1)], ids=["no_samples", "past_the_row", "negative_padding"])
def test_a_stream_without_a_body_inside_its_row_is_refused(monkeypatch, name, count, pad):
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    row = np.full((1, 64), 128, np.uint8)                     # 30 + 40 > 64
    w = WavStream.from_prepared(row, RATE, count, pad)
    with pytest.raises(SushiError) as e:
        METHODS[name](w)
    assert str(e.value) == "%s: the stream has no body inside its row" % name


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_every_derived_stream_is_adopted_live_and_laid_out_as_stated(monkeypatch, sample_type):
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    src = WavStream.from_samples(synth.make_dst_pcm(1, RATE, seed=5), RATE, sample_rate=RATE, sample_type=sample_type)
    rate, pad, count = src.sample_rate, src.padding_size, src.sample_count
    assert (rate, count) == (RATE, RATE) and pad == 20000
    cases = (
        (src.filtered(low=150), (rate, pad, count)),
        (src.envelope(8, 4), (rate // 8, pad // 8, -(-count // 8))),
        (src.retimed(SPEED), (rate, pad, ((count - 1) * SPEED.numerator) // SPEED.denominator + 1)),
        (src.retimed(1), (rate, pad, count)),
    )
    for new, layout in cases:
        assert new is not src and type(new) is WavStream
        assert (new.sample_rate, new.padding_size, new.sample_count) == layout
        n_pad, n_count = new.padding_size, new.sample_count
        assert new.data.dtype == src.data.dtype and new.data.shape == (1, 2 * n_pad + n_count)
        assert new._dev_row is None and new._dev is None and new._device is src._device
        assert (new.data[0, :n_pad] == new.data[0, n_pad]).all()
        assert (new.data[0, n_pad + n_count:] == new.data[0, n_pad + n_count - 1]).all()
        owner, off, length = _locate(new.get_substream(0.25, 0.75))
        assert owner is new and off == n_pad + int(new.sample_rate * 0.25)
        assert length == int(new.sample_rate * 0.75) - int(new.sample_rate * 0.25)
    assert cases[3][0].data.tobytes() == src.data.tobytes()     # retimed(1) holds the same samples
