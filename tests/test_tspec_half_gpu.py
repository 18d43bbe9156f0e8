"""The half rows the real route stores of the pattern segments' spectra (tspec_real_kernel; fft_core.hpp "HALF ROWS") and every
reader of them, on the MI355X: the stored half rows against the whole-row view expanded from them, that view against float64,
the rows mac_rows_kernel's paired first pass forms (a stored entry and its mirror from one read of the spectra) against the rows of
the routes that take the pattern words entry by entry -- mac_list_kernel (SUSHI_HIP_PILOT_ROWS=list), the survivors' pass by search
(SUSHI_HIP_REST_ROWS=search), the dense mac_kernel (no exclusion) --, and a whole batch under SUSHI_HIP_TSPEC=real and complex.

The job: the pattern lengths of tests/test_tspec_real_gpu.py and one pattern of 7 segments (class 12) and one of 19 (the LONG
forms of mac_rows_kernel), cut from audio-like material (sushi_amd.synth, the source = the stream advanced plus noise) -- among a
crowd of two dozen events of 1 - 5 s as tests/test_pair_exclusion.py's _audio_like_job has them: exclusion="always" takes the
band-split form, the one with a first pass, only where three quarters of the batch's PAIRS leave its bound room (run_policy.hpp
decide_form), and patterns of a few samples leave none (58 pairs of these patterns alone: 9 votes, measured).  The streams are as
long as that crowd needs.  One sub-batch (asserted).  Which whole rows a run wrote: the sentinel procedure of the stage tests."""
import functools

import numpy as np
import pytest

import fft_stage_ref as R
import test_fft_stages_gpu as S          # material, pair geometry
import test_pilot_audit_rows_gpu as P    # the sentinel runs
from test_tspec_real_gpu import LENS as REAL_LENS

pytestmark = pytest.mark.gpu
PAIR = S.PAIR
LENS = list(REAL_LENS) + [7 * R.B - 777, 19 * R.B - 777]
HALF_STORED = R.N // 8                    # stored entries u < 2 of a half row (fft_core.hpp)
HALF_ROWE = HALF_STORED + 16              # ... and the run whose first two entries are row 1024's
METHOD = "sqdiff_normed"
CROWD = 24                                # events of the crowd


def conj_word(w):
    """fft_core.hpp real_conj_word: the sign of the imaginary half flipped, a zero imaginary half kept as it is"""
    return np.where((w & np.uint32(0x7FFF0000)) != 0, w ^ np.uint32(0x80000000), w)


@functools.lru_cache(maxsize=None)
def _job(dtype):
    """-> (dst WavStream, src WavStream, the source's samples as the device holds them, offs, lens, wst, npos)"""
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    rate, off, seconds, window = 12000, 2.25, 240.0, 40.0
    shift = int(off * rate)
    dst_pcm = synth.make_dst_pcm(seconds, rate, seed=71)
    src_pcm = synth.make_src_pcm(dst_pcm, shift, seed=72)
    sample_type = "uint8" if dtype == "u8" else "float32"
    dst = WavStream.from_samples(dst_pcm, rate, sample_rate=rate, sample_type=sample_type)
    src = WavStream.from_samples(src_pcm, rate, sample_rate=rate, sample_type=sample_type)
    hd, hs = [np.asarray(w.data.cpu().numpy() if hasattr(w.data, "cpu") else w.data).reshape(-1) for w in (dst, src)]
    # the crowd: events as the bench has them, whose pairs carry the vote
    events = synth.make_events(CROWD, seconds, window + off, seed=73)
    pats, centres, wins = synth.explicit_descriptors(src, dst, events, off, window, seed=74)
    offs = [src._get_sample_for_time(s) for s, _ in events]
    lens = [p.shape[1] for p in pats]
    wst, npos = [], []
    for m, c, w in zip(lens, centres, wins):
        _, lo, p = dst._window(m, c, w)
        wst.append(lo); npos.append(p)
    # the patterns this test is about: windows of two pairs for those of a segment or less, of eight for the others
    rng = np.random.default_rng(75)
    for k, m in enumerate(LENS):
        o = 100000 + 200000 * k
        ws = o + shift - int(rng.integers(PAIR, 3 * PAIR))
        p = (1 if m <= R.B + 1 else 7) * PAIR + 123
        offs.append(o); lens.append(m); wst.append(ws); npos.append(p)
        assert ws >= 0 and ws + p + m - 1 <= hd.shape[0] and o + m <= hs.shape[0]
    hs.setflags(write=False)
    return dst, src, hs, offs, lens, wst, npos


@functools.lru_cache(maxsize=None)
def _streams(dtype):
    job = _job(dtype)
    return job[0].device_stream(), job[1].device_stream()


def _batch(dtype, exclusion):
    from sushi_amd.device import SearchBatch
    D, Sx = _streams(dtype)
    _, _, _, offs, lens, wst, npos = _job(dtype)
    return SearchBatch(D, Sx, offs, lens, wst, npos, path="fft", method=METHOD, exclusion=exclusion)


@pytest.fixture(scope="module")
def lib():
    from sushi_amd import _native
    L = _native.lib()
    assert (L.sushi_hip_fft_size(), L.sushi_hip_fft_block()) == (R.N, R.B)
    return L


@pytest.fixture(scope="module")
def maps(lib):
    return R.slot_maps(lib)


def _clear_switches(monkeypatch):
    for name in ("SUSHI_HIP_TSPEC", "SUSHI_HIP_PILOT_ROWS", "SUSHI_HIP_REST_ROWS", "SUSHI_HIP_TEST_BOUND_FAULT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SUSHI_HIP_AUDIT_EVERY", "1")


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_stored_half_rows_are_the_expanded_views_entries_and_the_view_holds_its_reference(lib, maps, monkeypatch, dtype):
    from sushi_amd import _native
    slot, _ = maps
    _clear_switches(monkeypatch)
    _, _, src, offs, lens, wst, npos = _job(dtype)
    b = _batch(dtype, "always")
    b.run()
    assert b.sub_batches == 1
    uw = R.words(b.workspace_view(_native.WS_TSPEC), R.N).copy()
    hw = R.words(b.workspace_view(_native.WS_TSPEC_HALF), 4 * HALF_ROWE).copy()
    assert uw.shape[0] == hw.shape[0] == b.fft_segs == sum(-(-m // R.B) for m in lens)
    ue, he = uw.reshape(-1, R.N // 4, 4), hw.reshape(-1, HALF_ROWE, 4)
    # the stored entries: the whole row's entries whose index has bit 4 clear (u < 2), in order
    e = np.arange(R.N // 4)
    stored = e[(e & 16) == 0]
    assert (((stored >> 5) << 4) | (stored & 15)).tolist() == list(range(HALF_STORED))
    entry_of = lambda row, u: int(slot[row + 4096 * u]) // 4
    assert all(((entry_of(row, u) & 16) != 0) == (u >= 2) for row in (0, 1, 511, 512, 513, 1023) for u in range(4))
    assert (he[:, :HALF_STORED] == ue[:, stored]).all()
    # row 0's extras: the conj-reversals of its entries 3 and 2
    for x, u in ((0, 3), (1, 2)):
        assert (he[:, HALF_STORED + x] == conj_word(ue[:, entry_of(0, u)][:, ::-1])).all(), x
    # ... which are its own bins 1024 .. 7168 and bin N/2 as they stand
    nat = uw[:, slot]
    assert (he[:, HALF_STORED:HALF_STORED + 2].reshape(-1, 8) == nat[:, 1024 * np.arange(1, 9)]).all()
    # the expanded view is conjugate-symmetric word for word, and holds its float64 reference
    k = np.arange(1, R.N // 2)
    assert (nat[:, R.N - k] == conj_word(nat[:, k])).all() and not (nat[:, [0, R.N // 2]] >> 16).any()
    s0 = 0
    for o, m in zip(offs, lens):
        ref = R.pattern_spectra_ref(src[o:o + m], METHOD)
        ns = ref.shape[0]
        u = R.decode_rows(uw[s0:s0 + ns], slot)
        sc = R.infer_scale(u, ref, "U")
        assert sc is not None, m
        bad = R.spectrum_mismatch(u, ref, sc)
        assert bad is None, ("U", m, bad)
        s0 += ns
    assert s0 == uw.shape[0]


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_paired_first_pass_rows_are_every_other_routes_rows(lib, monkeypatch, dtype):
    """With the exclusion on and every search audited: the pilots' and audit pairs' rows of the default run (paired ROWS_FIRST; the
    survivors' by item) equal, word for word, the rows under SUSHI_HIP_PILOT_ROWS=list (mac_list_kernel, entry by entry) and under
    SUSHI_HIP_REST_ROWS=search; the dense mac_kernel's rows of the same pairs (no exclusion) equal them too."""
    from sushi_amd import _native
    _clear_switches(monkeypatch)
    geo = []
    pr0 = 0
    for w, p, m in zip(*_job(dtype)[5:7], _job(dtype)[4]):
        _, n_pairs, n_seg = S._pairs_of(lib, w, p, m)
        geo.append((pr0, n_pairs, n_seg))
        pr0 += n_pairs
    assert [s for _, _, s in geo][-2:] == [7, 19] and len(geo) == CROWD + len(LENS)
    got = {}
    for route, name, value in (("default", None, None), ("list", "SUSHI_HIP_PILOT_ROWS", "list"), ("search", "SUSHI_HIP_REST_ROWS", "search")):
        _clear_switches(monkeypatch)
        if name:
            monkeypatch.setenv(name, value)
        b = _batch(dtype, "always")
        (seq, res, d, written, yw), = P._sentinel_runs(b, 1)
        assert d["slb_violations"] == 0, (route, d)                 # (the patterns of a sample or two are tie-saturated: flagged, and answered by the tiles)
        got[route] = (res, written, yw.copy(), d)
    _clear_switches(monkeypatch)
    res, written, yw, d = got["default"]
    # the first pass's rows exist: a pilot's per search, and every search's audit pair's (all patterns here go through mac_rows_kernel)
    for g, (p0, n_pairs, n_seg) in enumerate(geo):
        assert written[p0:p0 + n_pairs].any(), g
        assert written[p0 + P.audit_pair(g, 1, n_pairs)], (g, P.audit_pair(g, 1, n_pairs))
    assert not written.all()                                        # (the bound excludes: rows are left untouched)
    audit_rows = {p0 + P.audit_pair(g, 1, n_pairs) for g, (p0, n_pairs, _) in enumerate(geo)}
    for route in ("list", "search"):
        res_o, written_o, yw_o, d_o = got[route]
        assert res_o == res, route
        print("\nhalf rows %s %s: rows written %d (default %d), only here %s, only in the default %s" % (
            dtype, route, int(written_o.sum()), int(written.sum()), np.flatnonzero(written_o & ~written).tolist(),
            np.flatnonzero(written & ~written_o).tolist()))
        both = written & written_o
        assert (yw[both] == yw_o[both]).all(), (route, np.flatnonzero((yw[both] != yw_o[both]).any(axis=1)))
        # the same rows exist -- but for what tests/test_pilot_audit_rows_gpu.py describes: the first pass also forms an audit pair
        # that the first bound keeps and the second look then drops, which the list route never forms
        only_default = np.flatnonzero(written & ~written_o)
        assert not (written_o & ~written).any(), route
        assert set(only_default.tolist()) <= (audit_rows if route == "list" else set()), (route, only_default.tolist())
    never = _batch(dtype, "never")
    never.run()
    assert never.sub_batches == 1 and P._result(never) == res
    yw_n = R.words(never.workspace_view(_native.WS_Y), R.N)
    assert yw_n.shape == yw.shape
    assert (yw_n[written] == yw[written]).all(), np.flatnonzero((yw_n[written] != yw[written]).any(axis=1))


@pytest.mark.parametrize("dtype", ["f32", "u8"])
def test_both_routes_answer_the_same_and_the_complex_route_has_no_half_rows(lib, monkeypatch, dtype):
    from sushi_amd import _native
    got = {}
    for route in ("real", "complex"):
        _clear_switches(monkeypatch)
        monkeypatch.setenv("SUSHI_HIP_TSPEC", route)
        b = _batch(dtype, "always")
        b.run()
        assert b.sub_batches == 1
        got[route] = P._result(b)
        if route == "complex":
            with pytest.raises(Exception):
                b.workspace_view(_native.WS_TSPEC_HALF)
            whole = b.workspace_view(_native.WS_TSPEC)                # (the stored rows themselves)
            assert R.words(whole, R.N).shape[0] == b.fft_segs
        else:
            assert R.words(b.workspace_view(_native.WS_TSPEC_HALF), 4 * HALF_ROWE).shape[0] == b.fft_segs
    assert got["real"] == got["complex"]
