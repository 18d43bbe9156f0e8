"""Each stage of the FFT path against float64, on material where "every fourth bin" and "the first bin four times" are badly wrong
(tones at chosen bins, level steps between blocks, bursts of a tone at Fs/8), and every block pair's lower bound against the oracle.
The references and the comparators -- with the derivation of every allowance -- are tests/fft_stage_ref.py; tests/test_fft_stage_ref.py
shows on the CPU that they reject the known failure modes.  Every stage is judged from the stored halves of the stage before it.
One sub-batch per batch (asserted), so that a workspace view covers every pair."""
import os
import sys

import numpy as np
import pytest

import fft_stage_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR = R.STEP * R.B


@pytest.fixture(scope="module")
def lib():
    from sushi_amd import _native
    L = _native.lib()
    assert (L.sushi_hip_fft_size(), L.sushi_hip_fft_block()) == (R.N, R.B)
    return L


@pytest.fixture(scope="module")
def maps(lib):
    return R.slot_maps(lib)


def _tone_bins(slot, lslot):
    """A bin at every sub-position j of a whole-row entry and of a low-row entry, the band's edges N/8 - 1, N/8, N/8 + 1 (their
    mirrors 7N/8 + 1, 7N/8, 7N/8 - 1 come with them: Z packs two real blocks), N/2 and bin 1."""
    out = []
    for j in range(4):
        out.append(int(next(f for f in range(300, R.N // 2) if slot[f] % 4 == j)))
        out.append(int(R.LOW_BINS[next(i for i in range(40, len(R.LOW_BINS) - 40) if lslot[i] % 4 == j)]))
    return out + [R.LOW - 1, R.LOW, R.LOW + 1, R.N // 2, 1]


def _unit(kind, n, seed, bins):
    """Material in [0, 1]."""
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == "tones":
        x = np.full(n, 0.5)
        for k, f in enumerate(bins):
            x += 0.01 * (1 + 0.3 * k) * np.cos(2 * np.pi * f * t / R.N + rng.uniform(0, 2 * np.pi))
        return x
    if kind == "steps":                  # a level per block (bin 0 dominates every row), a faint tone on top
        lv = rng.uniform(0.1, 0.9, n // R.B + 1)
        return np.clip(lv[t // R.B] + 0.01 * np.cos(2 * np.pi * bins[0] * t / R.N), 0, 1)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bound_hunt
    return bound_hunt.make("fs8burst", n, rng)


def _as(x, dtype, mag):
    return (x * 255 + 0.5).astype(np.uint8) if dtype == "u8" else (x * mag).astype(np.float32)


SAMPLES = [("u8", 1.0), ("f32", 1.0), ("f32", 300.0), ("f32", 1e-3)]


# ----------------------------------------------------------------------------------------------------------------- 1. stream spectra

@pytest.mark.parametrize("kind", ["tones", "steps", "fs8burst"])
@pytest.mark.parametrize("dtype,mag", SAMPLES)
def test_stream_spectra_low_rows_and_rest_norms(lib, maps, kind, dtype, mag):
    import torch
    from sushi_amd import _native
    from sushi_amd.device import DeviceStream
    slot, lslot = maps
    x = _as(_unit(kind, 9 * R.B + 1111, 11, _tone_bins(slot, lslot)), dtype, mag)
    d = DeviceStream(x)
    zw = R.words(d.spectra(), R.N)
    z = R.decode_rows(zw, slot)
    ref = R.block_spectra_ref(x)
    assert z.shape == ref.shape and not zw[-1].any()
    _, e7 = R.stream_stats(x)
    zs = R.infer_scale(z[:-1], ref[:-1], "Z")
    R.assert_scale_is(zs, *R.z_scale_arg(e7), what="Z")
    assert 32 <= np.abs(z[:-1]).max() <= 32768 * 1.001               # the stored range test_fft_spectra_match_numpy asserts
    bad = R.spectrum_mismatch(z, ref, zs)
    assert bad is None, ("Z", bad)
    low = R.words(d._view(_native.VIEW_SPECTRA_LOW, torch.float16), R.LOW_WORDS)
    bad = R.low_row_mismatch(low, lslot, ref, zs)
    assert bad is None, ("Z low", bad)
    # the three norms outside the band: upper bounds of the float64 norms of the stored halves, by at most their float32 sums'
    # worst case (spectra_kernel: per thread 12 dot2 = 24 roundings, then 6 in the wave and 16 over the waves -> gamma_46 of the
    # energy, half of it on the root; A and B: two more per term for the sums Z(f) +- conj Z(N-f) and the squares -> gamma_80),
    # the root and the product by the kernel's own factor one rounding each
    norms = d._view(_native.VIEW_ZNORM_REST, torch.float32).cpu().numpy().astype(np.float64).reshape(3, -1)[:, :z.shape[0]]
    for got, want, fac, n in zip(norms, R.rest_norms64(z), (1.000002, 1.000004, 1.000004), (46, 80, 80)):
        assert (got >= want).all(), (got - want).min()
        assert (got <= want * fac * (1 + R.gamma(n) / 2 + 2 * R.U24)).all(), (got / np.maximum(want, 1e-300)).max()


# ----------------------------------------------------------------------------------------------------------------- 2. pattern spectra

@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
@pytest.mark.parametrize("dtype,mag", SAMPLES)
def test_pattern_spectra(lib, maps, method, dtype, mag):
    from sushi_amd import _native
    from sushi_amd.device import DeviceStream, SearchBatch
    slot, lslot = maps
    bins = _tone_bins(slot, lslot)
    dst = _as(_unit("tones", 12 * R.B, 21, bins), dtype, mag)
    src = _as(_unit("tones", 8 * R.B, 22, bins[::-1]), dtype, mag)
    lens = [1, 4095, 4096, 4097, 2 * R.B + 5, 3 * R.B + 4000, 5 * R.B + 17]
    offs = [3, 100, 0, 7, 1234, 50, 2000]
    b = SearchBatch(DeviceStream(dst), DeviceStream(src), offs, lens, [0] * 7, [len(dst) - m - 100 for m in lens],
                    path="fft", method=method, exclusion="never")
    b.run()
    assert b.sub_batches == 1
    uw = R.words(b.workspace_view(_native.WS_TSPEC), R.N)
    lw = R.words(b.workspace_view(_native.WS_TSPEC_LOW), R.LOW_WORDS)
    s0 = 0
    for o, m in zip(offs, lens):
        t = src[o:o + m]
        ref = R.pattern_spectra_ref(t, method)
        ns = ref.shape[0]
        u = R.decode_rows(uw[s0:s0 + ns], slot)
        tn, tn_c, _, flat = R.templ_norms(t)
        sc = R.infer_scale(u, ref, "U")
        if sc is None:                                     # a pattern without variance, centred: nothing but zeros
            assert method == "ccoeff_normed" and flat and not uw[s0:s0 + ns].any() and not lw[s0:s0 + ns].any()
        else:
            R.assert_scale_is(sc * R.N, *R.t_scale_arg(tn_c if method == "ccoeff_normed" and not flat else tn), what="U")
            bad = R.spectrum_mismatch(u, ref, sc)
            assert bad is None, ("U", m, bad)
            bad = R.low_row_mismatch(lw[s0:s0 + ns], lslot, ref, sc)
            assert bad is None, ("U low", m, bad)
        s0 += ns
    assert s0 == uw.shape[0] == b.fft_segs


# ----------------------------------------------------------------------------------------------------------------- 3, 4. products and the bound's inputs

SEGS = [1, 6, 7, 12, 13, 18, 19, 24, 25, 30, 31, 36, 37, 74]      # every mac_class boundary; beyond 30: accumulating passes


def _product_job(dtype, slot, lslot):
    bins = _tone_bins(slot, lslot)
    n = 74 * R.B + 5 * PAIR
    rng = np.random.default_rng(31)
    lp = np.convolve(rng.standard_normal(n + 7), np.ones(8) / 8, "valid")
    x = np.clip(_unit("tones", n, 31, bins) + 0.1 * lp, 0, 1)          # tones on low-passed noise: one place matches a pattern
    dst = _as(x, dtype, 1.0)
    src = _as(np.clip(x + 0.002 * rng.standard_normal(n), 0, 1), dtype, 1.0)   # the patterns: the stream again, a little noise on it
    offs, lens, wst, npos = [], [], [], []
    for k, s in enumerate(SEGS):
        m = s * R.B - (100 if s > 1 else 1000)             # the last segment short
        ws = 5000 + 777 * k                                # windows off the pair grid at both ends
        p = 2 * PAIR + 1234 + 99 * k
        if s == 13:
            p = n - m - ws + 1                             # ... and one that reaches the end of the stream
        offs.append(ws + 3000 + 50 * k); lens.append(m); wst.append(ws); npos.append(p)   # the match inside the window's first pair
    # the search the band-split form takes densely: a pattern unrelated to the stream over many pairs
    noise = _as(rng.random(20000), dtype, 1.0)
    src = np.concatenate([src, noise])
    offs.append(len(src) - 20000); lens.append(20000); wst.append(3); npos.append(12 * PAIR)
    return dst, src, offs, lens, wst, npos


def _pairs_of(lib, ws, p, m):
    import ctypes
    a, s = ctypes.c_int32(0), ctypes.c_int32(0)
    assert lib.sushi_hip_fft_layout(int(ws), int(p), int(m), ctypes.byref(a), ctypes.byref(s)) == 0
    return (ws // R.B) // R.STEP, a.value, s.value


def _check_products(lib, job, y_words, z_c, u_c, what, rows=None, scales=None):
    """Every product row (or those with rows[pr] set) against mac_scale * sum_s conj(U_s) Z_{6g+s} of the stored factors; the
    scale one power of two per search, equal to the host's y_scale / (t_scale z_scale)."""
    dst, src, offs, lens, wst, npos = job
    pr0, s0, checked = 0, 0, 0
    for k in range(len(offs)):
        pair0, n_pairs, n_seg = _pairs_of(lib, wst[k], npos[k], lens[k])
        refs, mags, got = [], [], []
        for i in range(n_pairs):
            if rows is None or rows[pr0 + i]:
                partials, mag = R.product_terms(u_c[s0:s0 + n_seg], z_c, pair0 + i)
                refs.append(partials); mags.append(mag); got.append(R.complex_of_words(y_words[pr0 + i]))
        if refs:
            ms = R.infer_scale(np.array(got), np.array([p[-1] for p in refs]), what)
            if scales is not None and ms is not None:
                assert ms == scales[k], (what, k, ms, scales[k])
            for y, p, mag in zip(got, refs, mags):
                bad = R.product_mismatch(y, p, mag, ms)
                assert bad is None, (what, k, n_seg, bad)
            checked += len(refs)
        pr0 += n_pairs
        s0 += n_seg
    return checked


def _host_mac_scales(job, method):
    dst, src, offs, lens, wst, npos = job
    _, e7 = R.stream_stats(dst)
    out = []
    for o, m in zip(offs, lens):
        tn, tn_c, _, flat = R.templ_norms(src[o:o + m])
        t = tn_c if method == "ccoeff_normed" and not flat else tn
        ns = -(-m // R.B)
        out.append(R.pow2_under(*R.y_scale_arg(t, ns, e7)) / (R.pow2_under(*R.t_scale_arg(t)) * R.pow2_under(*R.z_scale_arg(e7))))
    return out


def _assert_bound_inputs(b, form, model, y_nat, ylow_nat, y_words, ylow_words):
    """acc[:, 0] bounds what the kernel's header says from above, at every position; acc[:, 1] (statistical model) is the row
    energy the kernel defines, to its float32 sum's worst case."""
    slb, acc = b.pair_bounds()
    acc = acc.astype(np.float64)
    if form == "band":
        top = R.low_cross_term_max(ylow_nat)
        assert (acc[:, 0] >= top).all(), ("band acc0", int(np.argmin(acc[:, 0] - top)), (acc[:, 0] - top).min())
        if model == "statistical":
            # bound_low_kernel: lanes 0-31 each 8 groups x 4 entries x 4 dot2 (2 roundings each), a 6-level wave sum; x 1.000001
            e64 = (np.abs(R.complex_of_words(ylow_words)) ** 2).sum(axis=1)
            for pr in range(acc.shape[0]):
                ok, lim = R.energy_ok(acc[pr, 1], e64[pr], 2 * 128 + 6, 1.000001)
                assert ok, ("band acc1", pr, acc[pr, 1], lim)
    else:
        top = R.cross_term_modulus_max(y_nat)
        assert (acc[:, 0] >= top).all(), ("whole acc0", int(np.argmin(acc[:, 0] - top)), (acc[:, 0] - top).min())
        if model == "statistical":
            # bound_kernel: per wave 64 lanes x 4 entries x 4 dot2 (2 roundings each), a 6-level wave sum; the largest wave's
            we = R.wave_energies(y_words).max(axis=1)
            for pr in range(acc.shape[0]):
                ok, lim = R.energy_ok(acc[pr, 1], we[pr], 2 * 16 + 6, 1.0)
                assert ok, ("whole acc1", pr, acc[pr, 1], lim)
    return slb


def _band_sentinel_run(lib, b, job, z_c, zl_c, scales):
    """The band-split form's rows: every Y_LOW row (mac_kernel<LROWE> / mac_long_kernel<LROWE>) and the whole rows that exist.  Which
    whole rows a run wrote: run once, fill the Y view with NaN halves, run again, fetch the view again.  Then (a) the second run's
    results are the first's bit for bit (no stage read a row nobody wrote), (b) every row is all sentinel or fully written,
    (c) every written row matches its reference, (d) written rows >= pairs_transformed.  -> (diagnostics, written[pairs], Y_LOW words)."""
    import torch
    from sushi_amd import _native
    b.run()
    assert b.sub_batches == 1
    first = b.results()
    first = (first[0].copy(), first[1].copy().view(np.uint32))
    yv = b.workspace_view(_native.WS_Y)
    ptr, nb = yv.data_ptr(), yv.numel()
    yv.view(torch.int32).fill_(R.NAN_WORD)
    b.run()
    second = b.results()
    yv2 = b.workspace_view(_native.WS_Y)
    assert yv2.data_ptr() == ptr and yv2.numel() == nb                  # the same slice of the batch's memory
    assert (second[0] == first[0]).all() and (second[1].view(np.uint32) == first[1]).all()   # (a)
    d = b.diagnostics()
    assert d["band"] == 1
    yw = R.words(yv2, R.N)
    st = R.row_states(yw)
    assert (st != 2).all(), np.nonzero(st == 2)[0]                      # (b) never half-written
    written = st == 1
    assert written.sum() >= d["pairs_transformed"], (written.sum(), d["pairs_transformed"])     # (d)
    u_c = R.complex_of_words(R.words(b.workspace_view(_native.WS_TSPEC), R.N))
    ul_c = R.complex_of_words(R.words(b.workspace_view(_native.WS_TSPEC_LOW), R.LOW_WORDS))
    ylw = R.words(b.workspace_view(_native.WS_Y_LOW), R.LOW_WORDS)
    assert _check_products(lib, job, ylw, zl_c, ul_c, "Y low", scales=scales) == b.fft_pairs
    assert _check_products(lib, job, yw, z_c, u_c, "Y band", rows=written, scales=scales) == written.sum()   # (c)
    return d, written, ylw


def _band_bound_inputs(b, lslot, ylw):
    from sushi_amd import _native
    ylow_nat = R.decode_low_rows(ylw, lslot)
    for model in ("statistical", "worst_case"):
        b.set_bound_model(model)
        b.run()
        _assert_bound_inputs(b, "band", model, None, ylow_nat, None, ylow_words=R.words(b.workspace_view(_native.WS_Y_LOW), R.LOW_WORDS))


def _classes(lib, job):
    """Searches per mac_class (segments up to 6 / 12 / 18 / 24 / 30, beyond 30 in passes of 30) and the segments they hold: the
    batch's fft_segs by class."""
    dst, src, offs, lens, wst, npos = job
    count, segs = [0] * 5, [0] * 5
    for w, p, m in zip(wst, npos, lens):
        ns = _pairs_of(lib, w, p, m)[2]
        count[min(4, (ns - 1) // 6)] += 1
        segs[min(4, (ns - 1) // 6)] += ns
    return {"searches": count, "fft_segs": segs}


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_products_of_every_class_and_the_bound_inputs(lib, maps, method, dtype):
    """Patterns of 1 .. 74 segments, windows off the pair grid and one to the stream's end.  'never' and 'whole': every Y row of
    mac_kernel<ROWE> / mac_long_kernel<ROWE>; 'band': every Y_LOW row and -- on this material, whose tones correlate with every
    pair, so that nothing is excluded and every search is taken densely -- every whole row through the dense launch
    (test_band_form_whole_rows_of_listed_pairs takes the routes of listed pairs).  The bound kernels' inputs of both forms under
    both models."""
    import torch
    from sushi_amd import _native
    from sushi_amd.device import DeviceStream, SearchBatch
    slot, lslot = maps
    job = _product_job(dtype, slot, lslot)
    dst, src, offs, lens, wst, npos = job
    D, S = DeviceStream(dst), DeviceStream(src)
    z_c = R.complex_of_words(R.words(D.spectra(), R.N))
    zl_c = R.complex_of_words(R.words(D._view(_native.VIEW_SPECTRA_LOW, torch.float16), R.LOW_WORDS))
    scales = _host_mac_scales(job, method)
    report = {}
    # never / whole: every Y row, mac_kernel<ROWE> and mac_long_kernel<ROWE>
    for form in ("never", "whole"):
        b = SearchBatch(D, S, offs, lens, wst, npos, path="fft", method=method, exclusion=form)
        b.run()
        assert b.sub_batches == 1
        u_c = R.complex_of_words(R.words(b.workspace_view(_native.WS_TSPEC), R.N))
        yw = R.words(b.workspace_view(_native.WS_Y), R.N)
        assert yw.shape[0] == b.fft_pairs
        assert _check_products(lib, job, yw, z_c, u_c, "Y " + form, scales=scales) == b.fft_pairs
        d = b.diagnostics()
        report[form] = (d["band"], d["pairs_transformed"], b.fft_pairs)
        if form == "whole":
            y_nat = R.decode_rows(yw, slot)
            for model in ("statistical", "worst_case"):
                b.set_bound_model(model)
                b.run()
                _assert_bound_inputs(b, "whole", model, y_nat, None, yw, None)
    b = SearchBatch(D, S, offs, lens, wst, npos, path="fft", method=method, exclusion="band")
    d, written, ylw = _band_sentinel_run(lib, b, job, z_c, zl_c, scales)
    assert d["pairs_transformed"] == b.fft_pairs and written.all()     # (e) every search taken densely: all its pairs written
    report["band"] = (d["band"], d["pairs_transformed"], b.fft_pairs, int(written.sum()))
    _band_bound_inputs(b, lslot, ylw)
    print("\nproducts %s %s: %s; (band, pairs_transformed, pairs[, whole rows written]) %s" % (
        method, dtype, _classes(lib, job), report))


LISTED_SEGS = [5, 15, 20, 25, 35, 40]      # two searches per group: up to 18, 19 - 30, beyond 30 segments


def _listed_job(dtype):
    """Audio-like material (sushi_amd.synth: band-limited noise under a slow envelope; the source = the stream advanced by 27,000
    samples plus white noise at 20 dB) with one match per search, in windows of 16 pairs: the band-split bound excludes most pairs.
    Survivors of 5 and 15 segments go through mac_rows_kernel<0>, of 20 and 25 through mac_rows_kernel<1>, of 35 and 40 through
    mac_list_kernel (two accumulating passes)."""
    from sushi_amd import synth
    rate, shift = 12000, 27000
    dst_pcm = synth.make_dst_pcm(180, rate, seed=51)
    src_pcm = synth.make_src_pcm(dst_pcm, shift, seed=52)
    # the full range, as WavStream normalises: a quieter stream on the same level leaves TM_SQDIFF_NORMED's scores too little
    # spread for the bound to exclude anything (its scores of uncentred windows are all close to 0)
    dst = _as(np.clip(dst_pcm.astype(np.float64) / 32768.0 + 0.5, 0, 1), dtype, 1.0)
    src = _as(np.clip(src_pcm.astype(np.float64) / 32768.0 + 0.5, 0, 1), dtype, 1.0)
    rng = np.random.default_rng(53)
    offs, lens, wst, npos = [], [], [], []
    for k, s in enumerate(LISTED_SEGS):
        o = 200000 + 220000 * k
        m = s * R.B - 777
        ws = o + shift - int(rng.integers(PAIR, 6 * PAIR))
        offs.append(o); lens.append(m); wst.append(ws); npos.append(16 * PAIR + 123)
        assert ws >= 0 and ws + npos[-1] + m - 1 <= dst.shape[0] and o + m <= src.shape[0]
    return dst, src, offs, lens, wst, npos


# ----------------------------------------------------------------------------------------------------------------- 5. every pair's lower bound

def _oracle_rows(oracle, job, method):
    dst, src, offs, lens, wst, npos = job
    return [oracle.match_template(dst[w:w + p + m - 1], src[o:o + m], corr_f32=False, method=method)[0]
            for o, m, w, p in zip(offs, lens, wst, npos)]


def _assert_every_pair_bound(lib, job, slb, rows, method, what):
    """slb <= the smallest exact score over the pair's valid positions (ccoeff_normed: ranked as 1 - cc), slack one float32 ulp of
    that score; -inf allowed.  Scores are clamped to the method's range (cv2: sqdiff_normed <= 1, 1 - cc <= 2), so is the bound."""
    dst, src, offs, lens, wst, npos = job
    cap = 1.0 if method == "sqdiff_normed" else 2.0
    pr0 = 0
    for k in range(len(offs)):
        pair0, n_pairs, _ = _pairs_of(lib, wst[k], npos[k], lens[k])
        sc = rows[k].astype(np.float64) if method == "sqdiff_normed" else 1.0 - rows[k].astype(np.float64)
        for i in range(n_pairs):
            lo = max(0, (pair0 + i) * PAIR - wst[k])
            hi = min(npos[k], (pair0 + i + 1) * PAIR - wst[k])
            best = sc[lo:hi].min()
            ulp = float(np.spacing(np.float32(abs(best))))
            assert min(float(slb[pr0 + i]), cap) <= best + ulp, (what, k, i, float(slb[pr0 + i]), best)
        pr0 += n_pairs
    assert pr0 == slb.shape[0]


def _bound_job(kind, dtype, mag, seed):
    rng = np.random.default_rng(seed)
    n = 16 * PAIR
    x = _unit(kind, n, seed, [1234, R.LOW - 1, R.LOW, R.N // 2, 1])
    dst = _as(x, dtype, mag)
    offs, lens, wst, npos, parts, pos = [], [], [], [], [], 0
    for k, m in enumerate([300, 4096, 9000, 30000, 50000]):
        a = int(rng.integers(0, n - m))
        piece = dst[a:a + m].astype(np.float64)
        if k % 2:
            piece = piece + rng.standard_normal(m) * (3.0 if dtype == "u8" else 0.01 * mag)
        parts.append(np.clip(piece, 0, 255 if dtype == "u8" else None).astype(dst.dtype))
        w0 = int(rng.integers(0, max(1, a)))
        offs.append(pos); lens.append(m); wst.append(w0); npos.append(n - m - w0 + 1)
        pos += m
    return dst, np.concatenate(parts), offs, lens, wst, npos


@pytest.mark.parametrize("kind,dtype,mag", [("tones", "u8", 1.0), ("tones", "f32", 1.0), ("fs8burst", "u8", 1.0),
                                            ("fs8burst", "f32", 300.0), ("steps", "f32", 1e-3)])
def test_every_pairs_lower_bound_is_below_its_scores(lib, oracle, kind, dtype, mag):
    from sushi_amd.device import DeviceStream, SearchBatch
    job = _bound_job(kind, dtype, mag, 41)
    dst, src, offs, lens, wst, npos = job
    D, S = DeviceStream(dst), DeviceStream(src)
    for method in ("sqdiff_normed", "ccoeff_normed"):
        rows = _oracle_rows(oracle, job, method)
        for form in ("band", "whole"):
            b = SearchBatch(D, S, offs, lens, wst, npos, path="fft", method=method, exclusion=form)
            b.run()
            assert b.sub_batches == 1
            slb, _ = b.pair_bounds()
            assert b.diagnostics()["band"] == (form == "band")
            _assert_every_pair_bound(lib, job, slb, rows, method, (kind, dtype, mag, method, form))


def test_every_pairs_lower_bound_on_audio_like_material(lib, oracle):
    """The bench's kind of material: every pair's bound below its scores, and most bounds above the search's answer -- the check
    is not vacuous."""
    from test_pair_exclusion import _audio_like_job
    from sushi_amd.device import SearchBatch
    dst, src, offs, lens, wst, npos, planted = _audio_like_job()
    host = [np.asarray(w.data.cpu().numpy() if hasattr(w.data, "cpu") else w.data).reshape(-1) for w in (dst, src)]
    job = (host[0], host[1], offs, lens, wst, npos)
    for method in ("sqdiff_normed", "ccoeff_normed"):
        rows = _oracle_rows(oracle, job, method)
        for form in ("band", "whole"):
            b = SearchBatch(dst.device_stream(), src.device_stream(), offs, lens, wst, npos, path="fft", method=method, exclusion=form)
            b.run()
            assert b.sub_batches == 1
            idx, score = b.results()
            slb, _ = b.pair_bounds()
            _assert_every_pair_bound(lib, job, slb, rows, method, ("audio", method, form))
            answer = score.astype(np.float64) if method == "sqdiff_normed" else 1.0 - score.astype(np.float64)
            per_pair = np.concatenate([np.full(_pairs_of(lib, w, p, m)[1], a) for w, p, m, a in zip(wst, npos, lens, answer)])
            above = np.isfinite(slb) & (slb > per_pair)
            d = b.diagnostics()
            print("\naudio-like %s %s: %d of %d pairs bounded above their answer; band %d, pairs_transformed %d" % (
                method, form, int(above.sum()), slb.shape[0], d["band"], d["pairs_transformed"]))
            assert above.sum() > slb.shape[0] // 2, (method, form, int(above.sum()), slb.shape[0])


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_band_form_whole_rows_of_listed_pairs(lib, maps, oracle, monkeypatch, method, dtype):
    """The band-split form where its bound excludes most pairs: the whole rows of the pairs transformed first and of the survivors
    come from mac_list_kernel (every pilot; every listed pair of a pattern beyond 30 segments, in accumulating passes) and
    mac_rows_kernel<0> / <1> (survivors of up to 18 / 30 segments).  Every search is audited every run (SUSHI_HIP_AUDIT_EVERY=1:
    a hashed pair of it, if excluded, is transformed all the same), so a search has listed pairs beside its pilot.  The sentinel
    procedure shows which rows were written, and the routes are asserted reached: pairs excluded, rows left untouched, and in each
    group of segment counts (up to 18, 19 - 30, beyond 30) a search not taken densely (fewer than 2/5 of its pairs written) with
    at least two rows written.  Then the bound kernels' inputs (after the second look) and every pair's lower bound."""
    import torch
    from sushi_amd import _native
    from sushi_amd.device import DeviceStream, SearchBatch
    monkeypatch.setenv("SUSHI_HIP_AUDIT_EVERY", "1")                  # (read when a batch is created)
    slot, lslot = maps
    job = _listed_job(dtype)
    dst, src, offs, lens, wst, npos = job
    D, S = DeviceStream(dst), DeviceStream(src)
    z_c = R.complex_of_words(R.words(D.spectra(), R.N))
    zl_c = R.complex_of_words(R.words(D._view(_native.VIEW_SPECTRA_LOW, torch.float16), R.LOW_WORDS))
    b = SearchBatch(D, S, offs, lens, wst, npos, path="fft", method=method, exclusion="band")
    d, written, ylw = _band_sentinel_run(lib, b, job, z_c, zl_c, _host_mac_scales(job, method))
    assert d["pairs_transformed"] < b.fft_pairs and not written.all(), (d["pairs_transformed"], b.fft_pairs)
    pr0, per_search = 0, []
    for w, p, m in zip(wst, npos, lens):
        _, n_pairs, n_seg = _pairs_of(lib, w, p, m)
        per_search.append((n_seg, int(written[pr0:pr0 + n_pairs].sum()), n_pairs))
        pr0 += n_pairs
    for lo, hi in ((1, 18), (19, 30), (31, 1 << 30)):
        assert any(k >= 2 and 5 * k < 2 * n for s, k, n in per_search if lo <= s <= hi), (lo, hi, per_search)
    _band_bound_inputs(b, lslot, ylw)
    b.set_bound_model("worst_case")
    b.run()
    slb, _ = b.pair_bounds()
    _assert_every_pair_bound(lib, job, slb, _oracle_rows(oracle, job, method), method, ("listed", dtype, method))
    print("\nlisted pairs %s %s: %s; band %d, pairs_transformed %d of %d, whole rows written %d; (segments, rows written, pairs) "
          "per search %s" % (method, dtype, _classes(lib, job), d["band"], d["pairs_transformed"], b.fft_pairs, int(written.sum()),
                             per_search))
