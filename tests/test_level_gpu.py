"""Levelling on the GPU: sushi_hip_level against its NumPy restatement, bit for bit; the hand cases and the pinned order; every
refusal of the entry point; WavStream.levelled on both paths; the dub scenario of tests/level_cases.py through the real searches."""
import numpy as np
import pytest

import filter_cases as FC
import level_cases as LC
from sushi_amd import _native, level as LV

pytestmark = pytest.mark.gpu


def _device(x, in_start, window, floor, peak, out_len, lead=0, in_lead=0, stream=None):
    """level_device from a view that starts `in_lead` samples into its allocation into a view that starts `lead` samples into a
    buffer of lead + out_len + 8 samples; nothing outside the view may be written."""
    import torch
    x = np.ascontiguousarray(x)
    src = torch.empty(in_lead + x.shape[0], dtype=torch.from_numpy(x).dtype, device="cuda")
    src[in_lead:] = torch.from_numpy(x).cuda()
    t = src[in_lead:]
    fill = 77 if x.dtype == np.uint8 else -3.0
    buf = torch.full((lead + out_len + 8,), fill, dtype=t.dtype, device=t.device)
    if stream is None:
        LV.level_device(t, in_start, window, floor, peak, out_len, out=buf[lead:lead + out_len])
    else:
        torch.cuda.current_stream().synchronize()
        LV.level_device(t, in_start, window, floor, peak, out_len, out=buf[lead:lead + out_len], hip_stream=stream.cuda_stream)
        stream.synchronize()
    got = buf.cpu().numpy()
    assert (got[:lead] == fill).all() and (got[lead + out_len:] == fill).all()
    return got[lead:lead + out_len]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("window", LC.WINDOWS)
def test_level_device_equals_level_host_bitwise(dtype, window):
    import torch
    side = torch.cuda.Stream()
    tile = LC.launch_shape(dtype, window)[0]
    out_lens = (1, 2, tile - 1, tile, tile + 1)
    n = 0
    for n_in in LC.ROWS:
        x = FC.samples(n_in, dtype, seed=n_in)
        want = {}
        for in_start in LC.starts(n_in):
            for out_len in out_lens:
                # by turns: every (floor, peak), the views at their allocation's start or 1 or 3 samples inside it, the current
                # stream or a side stream
                pair = LC.PAIRS[n % len(LC.PAIRS)]
                if (in_start, pair) not in want:                       # an output does not depend on how many follow it
                    want[in_start, pair] = LV.level_host(x, in_start, window, pair[0], pair[1], max(out_lens))
                got = _device(x, in_start, window, pair[0], pair[1], out_len, lead=(0, 1, 3)[n % 3], in_lead=(3, 0, 1)[n % 3],
                              stream=side if n % 4 == 1 else None)
                n += 1
                w = want[in_start, pair][:out_len]
                assert got.tobytes() == w.tobytes(), (n_in, in_start, out_len, pair, int((got != w).sum()))
    pair = LC.PAIRS[0]
    got = LV.level_device(torch.from_numpy(x).cuda(), 0, window, pair[0], pair[1], 5).cpu().numpy()                # out=None
    assert got.tobytes() == LV.level_host(x, 0, window, pair[0], pair[1], 5).tobytes()


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("window", [3, 129])
def test_more_tiles_than_workgroups(dtype, window):
    """One tile and one output more than the launch has workgroups (1024): a workgroup takes a second tile, over what its first
    one staged.  The row has 70,001 samples; most outputs read past its end and see its last sample."""
    tile, most, _lds = LC.launch_shape(dtype, window)
    assert most == 1024
    x = FC.samples(70001, dtype, seed=window)
    out_len = (most + 1) * tile + 1
    got = _device(x, 12345, window, 1.0 / 128, 8.0, out_len, lead=3, in_lead=1)
    want = LV.level_host(x, 12345, window, 1.0 / 128, 8.0, out_len)
    assert got.tobytes() == want.tobytes(), int((got != want).sum())


def test_hand_cases_and_the_pinned_order():
    for x, in_start, window, floor, peak, want in LC.hand_cases():
        assert _device(x, in_start, window, floor, peak, len(want), lead=1).tolist() == want, (x, window, peak)
    x, in_start, window, floor, peak = LC.order_case()
    assert _device(x, in_start, window, floor, peak, 1).tolist() == [LC.ORDER_SEQUENTIAL]      # neither reversed nor pairwise


def test_every_refusal_through_the_native_call():
    """The entry point with real device memory: every refusal's return code, and nothing written."""
    import torch
    L = _native.lib()
    x = torch.full((1000,), 0.75, dtype=torch.float32, device="cuda")
    out = torch.full((104,), -3.0, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def call(n_in=1000, in_start=0, window=129, floor=1.0 / 128, peak=8.0, out_len=100, dtype=_native.F32, src=x.data_ptr(),
             dst=out.data_ptr()):
        return L.sushi_hip_level(src, dtype, n_in, in_start, window, floor, peak, dst, out_len, st)

    for kw in ({"src": None}, {"dst": None}, {"dtype": 2}, {"dtype": -1}, {"n_in": 0}, {"n_in": -5}, {"n_in": 1 << 62}, {"out_len": 0},
               {"out_len": -1}, {"out_len": 1 << 40}, {"in_start": -1}, {"in_start": 1000}, {"window": 0}, {"window": -3},
               {"window": 2}, {"window": 128}, {"window": 1024}, {"window": 1025}, {"floor": 0.0}, {"floor": -1.0},
               {"floor": float("inf")}, {"floor": float("nan")}, {"peak": 0.0}, {"peak": -8.0}, {"peak": float("inf")},
               {"peak": float("nan")}):
        assert call(**kw) == -1, kw
    for kw in ({"src": x.data_ptr() + 2}, {"dst": out.data_ptr() + 1}, {"src": x.data_ptr() + 1, "dst": out.data_ptr() + 2}):
        assert call(**kw) == -2, kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -3.0).all()
    assert call() == 0                                                  # ... and the call they were variations of runs
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert got[:100].tobytes() == LV.level_host(x.cpu().numpy(), 0, 129, 1.0 / 128, 8.0, 100).tobytes() and (got[100:] == -3.0).all()


def test_level_device_refuses_bad_arguments():
    import torch
    from sushi_amd.common import SushiError
    x = torch.zeros(100, dtype=torch.uint8).cuda()
    for in_start, window, floor, peak, out_len in ((-1, 3, 0.5, 1.0, 1), (100, 3, 0.5, 1.0, 1), (0, 2, 0.5, 1.0, 1), (0, 1025, 0.5, 1.0, 1),
                                                   (0, 3, 0.0, 1.0, 1), (0, 3, 0.5, float("nan"), 1), (0, 3, 0.5, 1.0, 0),
                                                   (0, 3, 0.5, 1.0, 1 << 40)):
        with pytest.raises(SushiError):
            LV.level_device(x, in_start, window, floor, peak, out_len)
    with pytest.raises(SushiError):
        LV.level_device(x.cpu(), 0, 3, 0.5, 1.0, 1)
    with pytest.raises(SushiError):
        LV.level_device(x, 0, 3, 0.5, 1.0, 4, out=torch.zeros(5, dtype=torch.uint8).cuda())
    with pytest.raises(SushiError):
        LV.level_device(x, 0, 3, 0.5, 1.0, 4, out=torch.zeros(4, dtype=torch.float32).cuda())


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_levelled_on_the_gpu_equals_the_host_path(monkeypatch, sample_type):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    rate = 12000
    w = WavStream.from_samples(synth.make_dst_pcm(15, rate, seed=9), rate, sample_type=sample_type)
    assert w._dev_row is not None                              # the load pipeline ran on the GPU
    kinds = ({}, {"window": 33}, {"window": 1023, "floor": 2.0 ** -20, "peak": 0.75})
    on_gpu = [w.levelled(**kw) for kw in kinds]
    chain = w.filtered(low=150).levelled()
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    for kw, g in zip(kinds, on_gpu):
        h = w.levelled(**kw)
        assert h._dev_row is None and g._dev_row is not None and g._dev_row.is_cuda
        assert g.data.dtype == h.data.dtype and g.data.shape == h.data.shape and g.data.tobytes() == h.data.tobytes()
        assert (g.sample_count, g.padding_size, g.sample_rate) == (h.sample_count, h.padding_size, h.sample_rate) == \
            (w.sample_count, w.padding_size, w.sample_rate)
        row = g._dev_row
        assert g.device_stream().raw.data_ptr() == row.data_ptr()                        # handed on: no upload
        assert g.device_stream().raw.cpu().numpy().tobytes() == h.data.tobytes()         # the row the searches read
    # it composes: a band removed first, equal to the same chain on the host path
    h = w.filtered(low=150).levelled()
    assert chain._dev_row is not None and h._dev_row is None
    assert chain.data.shape == h.data.shape and chain.data.tobytes() == h.data.tobytes()


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_levelling_gives_back_what_the_speech_hides_on_the_gpu(sample_type):
    """The scenario of tests/test_level_host.py through the real find_substreams: 24 of 24 events at the planted shift after
    levelled() on both streams."""
    dst, src = LC.stream("dst", sample_type), LC.stream("src", sample_type)
    assert dst._dev_row is not None
    evs = LC.events()

    def shifts(s, d):
        pats, centres, starts = FC.requests(s, evs)
        _scores, _times, pos = d.find_substreams(pats, centres, [LC.WINDOW] * len(pats), with_index=True, method=FC.SQ)
        return np.asarray(pos, np.int64) - d.padding_size - starts

    raw = shifts(src, dst)
    l_dst, l_src = dst.levelled(), src.levelled()
    assert l_dst._dev_row is not None
    got = shifts(l_src, l_dst)
    n_raw, n_levelled = int((raw == LC.OFFSET).sum()), int((got == LC.OFFSET).sum())
    print(sample_type, "plain", n_raw, "levelled", n_levelled)
    assert n_levelled == 24, got
