"""Loudness contours on the GPU: sushi_hip_envelope against its NumPy restatement, bit for bit; WavStream.envelope on both paths;
the scenarios of tests/envelope_cases.py through the real searches; find_coarse_fine."""
import numpy as np
import pytest

import envelope_cases as EC
from sushi_amd import envelope

pytestmark = pytest.mark.gpu
CC = "ccoeff_normed"
SHAPES = [(1, 1), (8, 4), (7, 2), (64, 16), (256, 16)]            # (hop, span)


def _device(x, in_start, hop, span, out_len, lead=0, stream=None):
    """envelope_device into a view that starts `lead` samples into a buffer; the buffer's first lead + out_len + 8 samples."""
    import torch
    t = torch.from_numpy(x).cuda()
    fill = 77 if x.dtype == np.uint8 else -3.0
    buf = torch.full((lead + out_len + 8,), fill, dtype=t.dtype, device=t.device)
    if stream is None:
        envelope.envelope_device(t, in_start, hop, span, out_len, out=buf[lead:lead + out_len])
    else:
        torch.cuda.current_stream().synchronize()
        envelope.envelope_device(t, in_start, hop, span, out_len, out=buf[lead:lead + out_len], hip_stream=stream.cuda_stream)
        stream.synchronize()
    got = buf.cpu().numpy()
    assert (got[:lead] == fill).all() and (got[lead + out_len:] == fill).all()          # nothing outside the view is written
    return got[lead:lead + out_len]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
@pytest.mark.parametrize("hop,span", SHAPES)
def test_envelope_device_equals_envelope_host_bitwise(dtype, hop, span):
    import torch
    tile = min(4096 // hop, 512)
    side = torch.cuda.Stream()
    for n_in in (1, 1000, 70001, 3000001):
        x = EC.samples(n_in, dtype, seed=n_in + hop)
        big = n_in > 100000
        for in_start in ((12345,) if big else sorted({0, min(3, n_in - 1), n_in - 1})):
            cover = (n_in - in_start + hop - 1) // hop
            # past the row's end; the long row: more tiles than the grid has workgroups, so that it strides
            out_len = max(cover + 2 * span + 37, 1030 * tile + 3) if big else cover + 2 * span + 37
            want = envelope.envelope_host(x, in_start, hop, span, out_len)
            for lead, stream in (((3, side),) if big else ((0, None), (1, None), (3, side))):
                got = _device(x, in_start, hop, span, out_len, lead, stream)
                assert got.tobytes() == want.tobytes(), (n_in, in_start, lead, int((got != want).sum()))
            if not big:                                    # an output that stops inside the row
                short = max(1, cover // 2)
                assert _device(x, in_start, hop, span, short, 1).tobytes() == want[:short].tobytes()


def test_envelope_device_hand_cases_and_the_pinned_order():
    assert _device(np.full(100, 128, np.uint8), 10, 8, 4, 20).tolist() == [0] * 20
    assert _device(np.zeros(100, np.uint8), 0, 8, 4, 20).tolist() == [255] * 20
    assert _device(np.array([128, 129, 130, 128, 128, 127, 128, 128, 126, 128, 128, 128], np.uint8), 0, 4, 1, 3).tolist() == [2, 1, 1]
    assert _device(np.array([0.5, 1.0, 0.0, 0.75], np.float32), 0, 2, 2, 3).tolist() == [0.625, 0.625, 0.5]
    # sequential sums (tests/envelope_cases.py order_case: a pairwise sum gives 2^30 + 128)
    assert _device(EC.order_case(), 0, 4, 1, 1).tolist() == [2.0 ** 30] and _device(EC.order_case(), 1, 1, 4, 1).tolist() == [2.0 ** 30]
    # the widest window of every kind
    for hop, span in ((64, 64), (1, 64), (256, 1), (3, 64)):
        x = EC.samples(9000, np.float32, seed=hop)
        assert _device(x, 5, hop, span, 300, 1).tobytes() == envelope.envelope_host(x, 5, hop, span, 300).tobytes()


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_wavstream_envelope_on_the_gpu_equals_the_host_path(monkeypatch, sample_type):
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    rate = 12000
    w = WavStream.from_samples(synth.make_dst_pcm(30, rate, seed=9), rate, sample_type=sample_type)
    assert w._dev_row is not None                              # the load pipeline ran on the GPU
    on_gpu = {hs: w.envelope(*hs) for hs in ((8, 4), (16, 3), (1, 1))}
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    for hs, g in on_gpu.items():
        h = w.envelope(*hs)
        assert h._dev_row is None and g._dev_row is not None and g._dev_row.is_cuda
        assert g.data.dtype == h.data.dtype and g.data.shape == h.data.shape and g.data.tobytes() == h.data.tobytes()
        assert (g.sample_count, g.padding_size, g.sample_rate) == (h.sample_count, h.padding_size, h.sample_rate)
        row = g._dev_row
        assert g.device_stream().raw.data_ptr() == row.data_ptr()                        # handed on: no upload
        assert g.device_stream().raw.cpu().numpy().tobytes() == h.data.tobytes()         # the row the searches read


def _gpu_shifts(src, dst, evs, scale=1.0):
    pats, centres, starts = EC.requests(src, dst, evs, scale)
    scores, _times, pos = dst.find_substreams(pats, centres, [EC.WINDOW] * len(pats), with_index=True, method=CC)
    return np.asarray(pos, np.int64) - dst.padding_size - starts, starts, np.asarray(scores)


@pytest.fixture(scope="module")
def contours():
    made = {}

    def get(name, sample_type):
        if (name, sample_type) not in made:
            s = EC.stream(name, sample_type)
            made[(name, sample_type)] = (s, s.envelope(EC.HOP, EC.SPAN))
        return made[(name, sample_type)]
    return get


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_contour_search_on_the_gpu(contours, sample_type):
    """The counts of tests/test_envelope_host.py through the real searches: 24 of 24 on the contours in every case; the waveform
    search places fewer than 3 of 24 where the polarity or the carrier differs."""
    dst, dst_env = contours("dst", sample_type)
    evs = EC.events()
    for name in EC.CASES:
        src, src_env = contours(name, sample_type)
        got, _starts, scores = _gpu_shifts(src_env, dst_env, evs)
        hits = int((np.abs(got - EC.OFFSET // EC.HOP) <= 1).sum())
        print(sample_type, name, "contour", hits, "worst coefficient %.3f" % float(scores.min()))
        assert hits == 24, (name, got)
        wave, _starts, _scores = _gpu_shifts(src, dst, evs)
        near = int((np.abs(wave - EC.OFFSET) <= EC.HOP).sum())
        print(sample_type, name, "waveform", near)
        assert near == 24 if name == "same" else near < 3, (name, near)


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_contour_of_a_sped_up_source_on_the_gpu(contours, sample_type):
    _dst, dst_env = contours("dst", sample_type)
    _src, src_env = contours("speed", sample_type)
    retimed = src_env.retimed(EC.SPEED)
    evs = EC.events(EC.SPEED)
    got, starts, _scores = _gpu_shifts(retimed, dst_env, evs, scale=float(EC.SPEED))
    true = np.array([s * float(EC.SPEED) * EC.RATE / EC.HOP for s, _e in evs])
    hits = int((np.abs(got + starts - true) <= 2).sum())
    print(sample_type, "speed", hits)
    assert hits == 24, got + starts - true


@pytest.mark.parametrize("sample_type", ["uint8", "float32"])
def test_find_coarse_fine(contours, sample_type):
    """'same': every fine shift is the shift of one plain waveform search over the whole +-20 s.  'inverted': every coarse shift
    is right and the fine score stays below 0.5 -- a bound that only keeps a lucky match out.  Measured on one MI355X: the largest
    fine score on 'inverted' is 0.052 for both sample types (the true place scores about -0.95 and the arg-max lies elsewhere in
    the +-4 ms), the smallest on 'same' 0.954."""
    dst, dst_env = contours("dst", sample_type)
    evs = EC.events()
    src, src_env = contours("same", sample_type)
    found = envelope.find_coarse_fine(src, dst, evs, EC.WINDOW, EC.HOP, EC.SPAN, src_env=src_env, dst_env=dst_env)
    plain, _starts, plain_scores = _gpu_shifts(src, dst, evs)
    print(sample_type, "same: smallest fine score %.4f" % float(found.fine_score.min()))
    assert (found.fine_samples == plain).all() and (plain == EC.OFFSET).all()
    assert (found.fine_shift == plain / float(EC.RATE)).all()
    assert (found.fine_score.view(np.uint32) == plain_scores.astype(np.float32).view(np.uint32)).all()
    assert (np.abs(found.coarse_samples - EC.OFFSET // EC.HOP) <= 1).all()
    assert (found.coarse_shift == found.coarse_samples * EC.HOP / float(EC.RATE)).all()
    assert found.fine_window == (EC.SPAN + 2) * EC.HOP / float(EC.RATE) and found.seconds > 0
    # enveloped here when not given: the same answers
    again = envelope.find_coarse_fine(src, dst, evs[:3], EC.WINDOW)
    assert (again.coarse_samples == found.coarse_samples[:3]).all() and (again.fine_samples == found.fine_samples[:3]).all()
    src, src_env = contours("inverted", sample_type)
    found = envelope.find_coarse_fine(src, dst, evs, EC.WINDOW, EC.HOP, EC.SPAN, src_env=src_env, dst_env=dst_env)
    print(sample_type, "inverted: largest fine score %.4f, smallest coarse score %.4f"
          % (float(found.fine_score.max()), float(found.coarse_score.min())))
    assert (np.abs(found.coarse_samples - EC.OFFSET // EC.HOP) <= 1).all()
    assert (found.fine_score < 0.5).all()
