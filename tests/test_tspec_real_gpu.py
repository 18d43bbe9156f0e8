"""Pattern-segment spectra from the real-input transform (tspec_real_kernel, the default) and from the complex transform it
replaces (SUSHI_HIP_TSPEC=complex: tspec_kernel), on the MI355X: both against float64 with the comparators of
tests/fft_stage_ref.py, the real route's rows conjugate-symmetric word for word, and a whole batch the same under both."""
import numpy as np
import pytest

import fft_stage_ref as R

pytestmark = pytest.mark.gpu
PAIR = R.STEP * R.B
CONJ = np.uint32(0x80000000)
ROUTES = ("real", "complex")

# pattern lengths: one and two samples, one short of a segment, a segment, a segment and one sample (an odd length whose last
# segment is one sample), lengths that end inside a third and a fourth segment, two segments and one sample, and -- the last
# pattern -- a segment and a half of a flat stretch of the source (TM_CCOEFF_NORMED: answered without its spectra, all zero)
LENS = [1, 2, 4095, 4096, 4097, 2 * R.B + 5, 3 * R.B + 4000, 2 * R.B + 1, R.B + R.B // 2]
OFFS = [3, 9, 100, 0, 7, 1234, 50, 2000, 7 * R.B + 10]
FLAT = (7 * R.B, 9 * R.B)           # the flat stretch of the source


@pytest.fixture(scope="module")
def lib():
    from sushi_amd import _native
    L = _native.lib()
    assert (L.sushi_hip_fft_size(), L.sushi_hip_fft_block()) == (R.N, R.B)
    return L


@pytest.fixture(scope="module")
def maps(lib):
    return R.slot_maps(lib)


def _material(dtype, n, seed, flat=None):
    """A level with tones at a few bins (bin 1, the band's edges, N/4, next to N/2) and noise on top, in [0, 1]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.full(n, 0.5)
    for k, f in enumerate([1, R.LOW - 1, R.LOW, R.LOW + 1, 1234, R.N // 4, R.N // 2 - 1]):
        x += 0.012 * (1 + 0.2 * k) * np.cos(2 * np.pi * f * t / R.N + rng.uniform(0, 2 * np.pi))
    x += 0.05 * rng.standard_normal(n)
    if flat:
        x[flat[0]:flat[1]] = 0.25
    x = np.clip(x, 0, 1)
    return (x * 255 + 0.5).astype(np.uint8) if dtype == "u8" else x.astype(np.float32)


def _spectra_under(monkeypatch, route, dst, src, method):
    """(whole-row words, low-row words, tnorm_rest) of every pattern segment under one setting of the switch."""
    import torch
    from sushi_amd import _native
    from sushi_amd.device import DeviceStream, SearchBatch
    monkeypatch.setenv("SUSHI_HIP_TSPEC", route)
    b = SearchBatch(DeviceStream(dst), DeviceStream(src), OFFS, LENS, [0] * len(LENS), [len(dst) - m - 100 for m in LENS],
                    path="fft", method=method, exclusion="never")
    b.run()
    assert b.sub_batches == 1
    uw = R.words(b.workspace_view(_native.WS_TSPEC), R.N).copy()
    lw = R.words(b.workspace_view(_native.WS_TSPEC_LOW), R.LOW_WORDS).copy()
    tn = b.workspace_view(_native.WS_TNORM_REST).view(torch.float32).cpu().numpy().astype(np.float64)
    assert uw.shape[0] == lw.shape[0] == tn.shape[0] == b.fft_segs == sum(-(-m // R.B) for m in LENS)
    return uw, lw, tn


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_pattern_spectra_of_both_routes(lib, maps, monkeypatch, method, dtype):
    slot, lslot = maps
    dst = _material(dtype, 12 * R.B, 61)
    src = _material(dtype, 10 * R.B, 62, FLAT)
    refs = [R.pattern_spectra_ref(src[o:o + m], method) for o, m in zip(OFFS, LENS)]          # float64, once for both routes
    rest = R.rest_bins()
    for route in ROUTES:
        uw, lw, tn = _spectra_under(monkeypatch, route, dst, src, method)
        s0 = 0
        for o, m, ref in zip(OFFS, LENS, refs):
            t = src[o:o + m]
            ns = ref.shape[0]
            u = R.decode_rows(uw[s0:s0 + ns], slot)
            tnorm, tnorm_c, _, flat = R.templ_norms(t)
            assert flat or o != OFFS[-1]                    # (a single sample is flat too)
            sc = R.infer_scale(u, ref, "U")
            if method == "ccoeff_normed" and flat:          # a pattern without variance, centred: nothing but zeros
                assert sc is None and not uw[s0:s0 + ns].any() and not lw[s0:s0 + ns].any() and not tn[s0:s0 + ns].any()
            else:
                R.assert_scale_is(sc * R.N, *R.t_scale_arg(tnorm_c if method == "ccoeff_normed" else tnorm), what="U")
                bad = R.spectrum_mismatch(u, ref, sc)
                assert bad is None, (route, "U", m, bad)
                bad = R.low_row_mismatch(lw[s0:s0 + ns], lslot, ref, sc)
                assert bad is None, (route, "U low", m, bad)
            # the low row holds the whole row's own words
            low_nat = uw[s0:s0 + ns][:, slot][:, R.LOW_BINS].copy()
            low_nat[:, R.LOW_BINS == R.N - R.LOW] = 0
            assert (lw[s0:s0 + ns][:, lslot] == low_nat).all(), (route, m)
            # tnorm_rest: the float32 sum of |re|^2 + |im|^2 of the stored halves outside the band.  Products of halves are exact in
            # float32 and every term is >= 0, so n chained additions err by at most gamma_n of the sum (fft_stage_ref.energy_ok).
            # n: a thread's chain is at most 13 dot2 of two additions each (complex route; the real route: 12, an addition of its two
            # rows' sums, two more for bin N/2 or a tail lane, the doubling exact), six more across the wave, sixteen atomic
            # additions of the waves' sums (eight on the real route): 26 + 6 + 16 = 48.
            e64 = (np.abs(u[:, rest]) ** 2).sum(axis=1)
            for r in range(ns):
                ok, span = R.energy_ok(tn[s0 + r], e64[r], 48, 1.0)
                assert ok, (route, m, r, tn[s0 + r], span)
            if route == "real":
                nat = uw[s0:s0 + ns][:, slot]
                k = np.arange(1, R.N // 2)
                # (the sign of the imaginary half flipped; a zero imaginary half kept as it is: fft_core.hpp real_conj_word)
                want = np.where((nat[:, k] & np.uint32(0x7FFF0000)) != 0, nat[:, k] ^ CONJ, nat[:, k])
                assert (nat[:, R.N - k] == want).all(), (m, "a mirror is not its bin's conjugate word for word")
                assert not (nat[:, [0, R.N // 2]] >> 16).any(), (m, "bins 0 and N/2 are real")
            s0 += ns
        assert s0 == uw.shape[0]


def _pairs_of(lib, ws, p, m):
    import ctypes
    a, s = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.sushi_hip_fft_layout(int(ws), int(p), int(m), ctypes.byref(a), ctypes.byref(s)) == 0
    return (ws // R.B) // R.STEP, a.value, s.value


def test_a_batch_is_answered_the_same_by_both_routes_and_every_pair_bound_holds(lib, oracle, monkeypatch):
    """40 searches of audio-like material through the band-split exclusion: the same indices and the same score bits under both
    settings, and under either every pair's lower bound at or below the smallest exact score over the pair's positions (the rule of
    tests/test_fft_stages_gpu.py's _assert_every_pair_bound: slack one float32 ulp of that score, -inf allowed, scores capped at 1)."""
    from test_pair_exclusion import _audio_like_job
    from sushi_amd.device import SearchBatch
    dst, src, offs, lens, wst, npos, planted = _audio_like_job()
    hd, hs = [np.asarray(w.data.cpu().numpy() if hasattr(w.data, "cpu") else w.data).reshape(-1) for w in (dst, src)]
    rows = [oracle.match_template(hd[w:w + p + m - 1], hs[o:o + m], corr_f32=False, method="sqdiff_normed")[0]
            for o, m, w, p in zip(offs, lens, wst, npos)]
    got = {}
    for route in ROUTES:
        monkeypatch.setenv("SUSHI_HIP_TSPEC", route)
        b = SearchBatch(dst.device_stream(), src.device_stream(), offs, lens, wst, npos, path="fft", exclusion="always")
        b.run()
        assert b.sub_batches == 1 and b.diagnostics()["band"] == 1
        idx, score = b.results()
        got[route] = (idx.copy(), score.copy().view(np.uint32))
        slb, _ = b.pair_bounds()
        pr0 = 0
        for k in range(len(offs)):
            pair0, n_pairs, _ = _pairs_of(lib, wst[k], npos[k], lens[k])
            sc = rows[k].astype(np.float64)
            for i in range(n_pairs):
                lo = max(0, (pair0 + i) * PAIR - wst[k])
                hi = min(npos[k], (pair0 + i + 1) * PAIR - wst[k])
                best = sc[lo:hi].min()
                ulp = float(np.spacing(np.float32(abs(best))))
                assert min(float(slb[pr0 + i]), 1.0) <= best + ulp, (route, k, i, float(slb[pr0 + i]), best)
            pr0 += n_pairs
        assert pr0 == slb.shape[0]
    assert (got["real"][0] == got["complex"][0]).all() and (got["real"][1] == got["complex"][1]).all()
    assert all(abs(int(i) - p) <= 1 for i, p in zip(got["real"][0], planted))


def test_an_unknown_route_is_refused(monkeypatch):
    from sushi_amd.device import DeviceStream, SearchBatch
    x = _material("f32", 4 * R.B, 63)
    monkeypatch.setenv("SUSHI_HIP_TSPEC", "cplx")
    with pytest.raises(Exception):
        SearchBatch(DeviceStream(x), DeviceStream(x), [0], [100], [0], [1000], path="fft")
