"""A stateless call on a stream of the caller's (sushi_amd.device._launch, through match_curves and retime_device): the bits of
the same call on the current stream.  Shapes: the smallest that cross a 1024-position tile edge and leave a partial wave."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _bytes(t):
    return t.cpu().numpy().view(np.uint8)


def test_match_curves_on_a_side_stream():
    import torch
    from sushi_amd.curves import match_curves
    from sushi_amd.device import DeviceStream
    row = np.random.default_rng(5).integers(0, 256, 8192, dtype=np.uint8)
    dst, src = DeviceStream(row), DeviceStream(row[::-1].copy())
    requests = ([100, 5000], [300, 300], [7, 3001], [1025, 63])
    want, want_off = match_curves(dst, src, *requests)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    got, got_off = match_curves(dst, src, *requests, hip_stream=side.cuda_stream)
    side.synchronize()
    assert list(got_off) == list(want_off) == [0, 1025, 1088]
    assert np.array_equal(_bytes(got), _bytes(want))
    assert float(want.min().item()) >= 0.0 and float(want.max().item()) > 0.0           # (a curve was written at all)


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_retime_device_on_a_side_stream(dtype):
    import torch
    from sushi_amd import retime
    rng = np.random.default_rng(6)
    x = rng.integers(0, 256, 4097, dtype=np.uint8) if dtype == np.uint8 else rng.random(4097, dtype=np.float32)
    dev = torch.from_numpy(x).cuda()
    segment = [(0, 0, 4097, 24, 25)]
    want = retime.retime_device(dev, segment)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = torch.empty(4097, dtype=dev.dtype, device=dev.device)
    got = retime.retime_device(dev, segment, out=out, hip_stream=side.cuda_stream)
    side.synchronize()
    assert got is out and np.array_equal(_bytes(got), _bytes(want))
    assert np.array_equal(_bytes(want), retime.retime_host(x, segment).view(np.uint8))
