"""Filtering on the GPU: sushi_hip_filter against its NumPy restatement, bit for bit; the hand cases and the pinned order;
WavStream.filtered on both paths; the hum scenario of tests/filter_cases.py through the real searches."""
import numpy as np
import pytest

import filter_cases as FC
from sushi_amd import _native, filter as F

pytestmark = pytest.mark.gpu


def _device(x, in_start, taps, out_len, lead=0, stream=None, taps_on_device=False):
    """filter_device into a view that starts `lead` samples into a buffer of lead + out_len + 8 samples; nothing outside the view
    may be written."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    h = np.asarray(taps, np.float64)
    if taps_on_device:
        h = torch.from_numpy(h).cuda()
    fill = 77 if x.dtype == np.uint8 else -3.0
    buf = torch.full((lead + out_len + 8,), fill, dtype=t.dtype, device=t.device)
    if stream is None:
        F.filter_device(t, in_start, h, out_len, out=buf[lead:lead + out_len])
    else:
        torch.cuda.current_stream().synchronize()
        F.filter_device(t, in_start, h, out_len, out=buf[lead:lead + out_len], hip_stream=stream.cuda_stream)
        stream.synchronize()
    got = buf.cpu().numpy()
    assert (got[:lead] == fill).all() and (got[lead + out_len:] == fill).all()
    return got[lead:lead + out_len]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("n_taps", FC.TAP_COUNTS)
def test_filter_device_equals_filter_host_bitwise(dtype, n_taps):
    import torch
    side = torch.cuda.Stream()
    h = FC.taps(n_taps)
    n = 0
    for n_in in FC.ROWS:
        x = FC.samples(n_in, dtype, seed=n_in)
        longest = max(m for _s, m in FC.grid(n_in))
        want = {}
        for in_start, out_len in FC.grid(n_in):
            if in_start not in want:                                   # an output does not depend on how many follow it
                want[in_start] = F.filter_host(x, in_start, h, longest)
            # by turns: the view at the buffer's start or inside it, the current stream or a side stream, taps from the host or
            # in device memory
            got = _device(x, in_start, h, out_len, lead=(0, 1, 3)[n % 3], stream=side if n % 4 == 1 else None, taps_on_device=n % 2 == 1)
            n += 1
            assert got.tobytes() == want[in_start][:out_len].tobytes(), (n_in, in_start, out_len, int((got != want[in_start][:out_len]).sum()))
    assert F.filter_device(torch.from_numpy(x).cuda(), 0, h, 5).cpu().numpy().tobytes() == want[0][:5].tobytes()      # out=None


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("n_taps", [3, 1027])
def test_more_tiles_than_workgroups(dtype, n_taps):
    """One tile and three outputs more than the launch has workgroups (1280 for both tap counts): a workgroup takes a second tile,
    over what its first one staged.  The row has 70,001 samples; most outputs read past its end and see its last sample."""
    tile, most = FC.launch_shape(n_taps)
    assert most == 1280
    x = FC.samples(70001, dtype, seed=n_taps)
    h = FC.taps(n_taps)
    out_len = (most + 1) * tile + 3
    got = _device(x, 12345, h, out_len, lead=3)
    want = F.filter_host(x, 12345, h, out_len)
    assert got.tobytes() == want.tobytes(), int((got != want).sum())


def test_hand_cases_and_the_pinned_order():
    for x, in_start, taps, want in FC.hand_cases():
        assert _device(x, in_start, taps, len(want), lead=1).tolist() == want, (x, taps)
    x, in_start, h = FC.order_case()
    assert _device(x, in_start, h, 1).tolist() == [FC.ORDER_SEQUENTIAL]          # neither reversed, pairwise nor contracted


def test_nan_tap_through_the_native_call():
    """filter_device refuses taps that are not finite; the library does not look at them, and its arithmetic is defined: a NaN sum
    gives 0 on uint8 (both comparisons of the finish fail) and NaN on float32."""
    import torch
    from sushi_amd.common import SushiError
    L = _native.lib()
    x = torch.tensor([0, 128, 255, 7], dtype=torch.uint8).cuda()
    for taps in ([np.nan], [0.0, np.nan, 0.0]):
        with pytest.raises(SushiError):
            F.filter_device(x, 0, np.array(taps), 4)
        with pytest.raises(SushiError):
            F.filter_device(x, 0, torch.tensor(taps, dtype=torch.float64).cuda(), 4)
        h = torch.tensor(taps, dtype=torch.float64).cuda()
        out = torch.full((4,), 77, dtype=torch.uint8).cuda()
        st = torch.cuda.current_stream().cuda_stream
        assert L.sushi_hip_filter(x.data_ptr(), _native.U8, 4, 0, h.data_ptr(), len(taps), out.data_ptr(), 4, st) == 0
        assert out.cpu().tolist() == [0, 0, 0, 0]
    xf = torch.tensor([0.25, 0.5], dtype=torch.float32).cuda()
    h = torch.tensor([np.nan], dtype=torch.float64).cuda()
    out = torch.zeros(2, dtype=torch.float32).cuda()
    assert L.sushi_hip_filter(xf.data_ptr(), _native.F32, 2, 0, h.data_ptr(), 1, out.data_ptr(), 2, torch.cuda.current_stream().cuda_stream) == 0
    assert bool(torch.isnan(out).all())


def test_filter_device_refuses_bad_arguments():
    import torch
    from sushi_amd.common import SushiError
    x = torch.zeros(100, dtype=torch.uint8).cuda()
    for in_start, taps, out_len in ((-1, [1.0], 1), (100, [1.0], 1), (0, [1.0, 1.0], 1), (0, [], 1), (0, np.ones(2049), 1),
                                    (0, [1.0], 0), (0, [1.0], 1 << 40), (0, [[1.0]], 1)):
        with pytest.raises(SushiError):
            F.filter_device(x, in_start, np.asarray(taps, np.float64), out_len)
    for bad in (torch.ones(3, dtype=torch.float32).cuda(), torch.ones(3, dtype=torch.float64), torch.ones(6, dtype=torch.float64).cuda()[::2]):
        with pytest.raises(SushiError):
            F.filter_device(x, 0, bad, 1)
    with pytest.raises(SushiError):
        F.filter_device(x.cpu(), 0, [1.0], 1)
    with pytest.raises(SushiError):
        F.filter_device(x, 0, [1.0], 4, out=torch.zeros(5, dtype=torch.uint8).cuda())


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_filtered_on_the_gpu_equals_the_host_path(monkeypatch, sample_type):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    rate = 12000
    w = WavStream.from_samples(synth.make_dst_pcm(15, rate, seed=9), rate, sample_type=sample_type)
    assert w._dev_row is not None                              # the load pipeline ran on the GPU
    kinds = ({"low": 150}, {"low": 300, "high": 3000, "stop": True}, {"taps": F.preemphasis_taps()})
    on_gpu = [w.filtered(**kw) for kw in kinds]
    contour, retimed = on_gpu[0].envelope(8, 4), on_gpu[0].retimed("25/24")
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    for kw, g in zip(kinds, on_gpu):
        h = w.filtered(**kw)
        assert h._dev_row is None and g._dev_row is not None and g._dev_row.is_cuda
        assert g.data.dtype == h.data.dtype and g.data.shape == h.data.shape and g.data.tobytes() == h.data.tobytes()
        assert (g.sample_count, g.padding_size, g.sample_rate) == (h.sample_count, h.padding_size, h.sample_rate) == \
            (w.sample_count, w.padding_size, w.sample_rate)
        row = g._dev_row
        assert g.device_stream().raw.data_ptr() == row.data_ptr()                        # handed on: no upload
        assert g.device_stream().raw.cpu().numpy().tobytes() == h.data.tobytes()         # the row the searches read
    # it composes: a band contour and a filtered stream on another clock, each equal to its host path
    h = w.filtered(low=150)
    for g2, h2 in ((contour, h.envelope(8, 4)), (retimed, h.retimed("25/24"))):
        assert g2._dev_row is not None and h2._dev_row is None
        assert (g2.sample_count, g2.padding_size, g2.sample_rate) == (h2.sample_count, h2.padding_size, h2.sample_rate)
        assert g2.data.shape == h2.data.shape and g2.data.tobytes() == h2.data.tobytes()


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_high_pass_gives_back_what_the_hum_hides_on_the_gpu(sample_type):
    """The counts of tests/test_filter_host.py through the real find_substreams: at most 16 of 24 events at the planted shift on
    the streams as captured, 24 of 24 after filtered(low=150) on both."""
    dst, src = FC.stream("dst", sample_type), FC.stream("src", sample_type)
    assert dst._dev_row is not None
    evs = FC.events()

    def shifts(s, d):
        pats, centres, starts = FC.requests(s, evs)
        _scores, _times, pos = d.find_substreams(pats, centres, [FC.WINDOW] * len(pats), with_index=True, method=FC.SQ)
        return np.asarray(pos, np.int64) - d.padding_size - starts

    raw = shifts(src, dst)
    f_dst, f_src = dst.filtered(low=FC.LOW, n_taps=FC.N_TAPS), src.filtered(low=FC.LOW, n_taps=FC.N_TAPS)
    assert f_dst._dev_row is not None
    got = shifts(f_src, f_dst)
    n_raw, n_filtered = int((raw == FC.OFFSET).sum()), int((got == FC.OFFSET).sum())
    print(sample_type, "unfiltered", n_raw, "filtered", n_filtered)
    assert n_filtered == 24, got
    assert n_raw <= 16, raw
