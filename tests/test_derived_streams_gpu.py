"""WavStream.retimed / envelope / filtered on the GPU, from each row a stream can hold (sushi_amd/wav.py _derive, _device_row): the
load pipeline's row, the mirror device_stream() made of it, or an upload of the host row.  Each result equals the host path's
byte for byte, keeps its row in HBM for the matching, and leaves its parent as it was.  The arithmetic on tile-sized shapes is
tests/test_retime_gpu.py's, test_envelope_gpu.py's and test_filter_gpu.py's."""
import pytest

from sushi_amd import synth
from sushi_amd.wav import WavStream

pytestmark = pytest.mark.gpu

RATE = 2000
METHODS = {
    "retimed": lambda w: w.retimed("25/24"),
    "envelope": lambda w: w.envelope(8, 4),
    "filtered": lambda w: w.filtered(low=150),
}
STATES = ("loaded", "mirrored", "uploaded")


def _load(sample_type):
    return WavStream.from_samples(synth.make_dst_pcm(1, RATE, seed=5), RATE, sample_rate=RATE, sample_type=sample_type)


@pytest.fixture(scope="module", params=["uint8", "float32"])
def streams(request):
    """The stream in each state of its row, and every method's host result (made once; nothing changes them)."""
    mp = pytest.MonkeyPatch()
    mp.setenv("SUSHI_HIP_LOAD", "host")
    try:
        host = _load(request.param)
        expected = {name: method(host) for name, method in METHODS.items()}
    finally:
        mp.undo()
    loaded = _load(request.param)                            # (a) fresh from the GPU load
    assert loaded._dev_row is not None and loaded._dev_row.is_cuda and loaded._dev is None
    assert loaded.data.tobytes() == host.data.tobytes() and loaded.padding_size == 20000 and loaded.sample_count == RATE
    mirrored = _load(request.param)                          # (b) after device_stream()
    mirrored.device_stream()
    assert mirrored._dev is not None and mirrored._dev_row is None
    uploaded = WavStream.from_prepared(host.data.copy(), host.sample_rate, host.sample_count, host.padding_size)   # (c) never on the device
    assert uploaded._dev is None and uploaded._dev_row is None
    return {"loaded": loaded, "mirrored": mirrored, "uploaded": uploaded}, expected


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("name", sorted(METHODS))
def test_derived_on_the_gpu_equals_the_host_path_from_every_row(streams, name, state):
    by_state, expected = streams
    w, h = by_state[state], expected[name]
    dev, dev_row = w._dev, w._dev_row
    mirror_ptr = None if dev is None else dev.raw.data_ptr()
    g = METHODS[name](w)
    assert w._dev is dev and w._dev_row is dev_row           # the parent is what it was
    assert mirror_ptr is None or w._dev.raw.data_ptr() == mirror_ptr
    assert h._dev_row is None
    assert (g.sample_rate, g.padding_size, g.sample_count) == (h.sample_rate, h.padding_size, h.sample_count)
    assert g.data.dtype == h.data.dtype and g.data.shape == h.data.shape and g.data.tobytes() == h.data.tobytes()
    row = g._dev_row
    assert row is not None and row.is_cuda and g._dev is None
    assert g.device_stream().raw.data_ptr() == row.data_ptr()                        # handed on: no upload
    assert g.device_stream().raw.cpu().numpy().tobytes() == h.data.tobytes()         # the row the searches read


def test_the_row_the_gpu_reads_is_the_one_the_stream_holds(streams):
    from sushi_amd.wav import torch_device
    by_state, _expected = streams
    dev = torch_device("cuda")
    loaded, mirrored, uploaded = (by_state[s] for s in STATES)
    assert loaded._device_row(dev).data_ptr() == loaded._dev_row.data_ptr()
    assert mirrored._device_row(dev).data_ptr() == mirrored._dev.raw.data_ptr()
    up = uploaded._device_row(dev)
    assert up.is_cuda and up.device == dev and up.cpu().numpy().tobytes() == uploaded.data.tobytes()
    assert uploaded._dev is None and uploaded._dev_row is None
