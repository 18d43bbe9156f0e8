"""The stage comparators of tests/fft_stage_ref.py have teeth (CPU only).  Stored rows are emulated in NumPy -- the float64 reference
times its power-of-two scale, rounded through np.float16 and placed by the library's slot maps -- on tone material, where "every
fourth bin" and "the first bin four times" are badly wrong rather than merely noisy.  Every comparator must ACCEPT the emulation
and REJECT each known failure mode: the hipcc 7.2 miscompile (an entry's four words all its word 0), the same in an accumulating
pass of a long pattern, a product missing a segment, conjugated pattern spectra, a scale off by two, a non-zero slot 7N/8 in a low
row, a row energy taken over every fourth bin x 4, a half-written row."""
import numpy as np
import pytest

import fft_stage_ref as R


@pytest.fixture(scope="module")
def maps():
    from sushi_amd import _native
    L = _native.lib()
    assert (L.sushi_hip_fft_size(), L.sushi_hip_fft_block()) == (R.N, R.B)
    return R.slot_maps(L)


def _tone_bins(slot, lslot):
    """For every sub-position j of an entry, a bin whose whole-row slot is 4k + j and one (inside the band) whose low-row slot is."""
    out = []
    for j in range(4):
        out.append(int(next(f for f in range(300, R.N // 2) if slot[f] % 4 == j)))
        out.append(int(R.LOW_BINS[next(i for i in range(40, len(R.LOW_BINS) - 40) if lslot[i] % 4 == j)]))
    return out + [R.LOW - 1, R.LOW, R.LOW + 1, R.N // 2, 1]


def _tones(n, bins, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    x = np.full(n, 0.5)
    for k, f in enumerate(bins):
        x += 0.02 * (1 + 0.3 * k) * np.cos(2 * np.pi * f * t / R.N + rng.uniform(0, 2 * np.pi))
    return x.astype(np.float32)


@pytest.fixture(scope="module")
def material(maps):
    slot, lslot = maps
    x = _tones(6 * R.B + 777, _tone_bins(slot, lslot), 1)
    z = R.block_spectra_ref(x)
    _, e7 = R.stream_stats(x)
    zs = R.pow2_under(*R.z_scale_arg(e7))
    return x, z, zs, e7


def test_block_spectra_emulation_is_accepted_and_the_miscompile_rejected(maps, material):
    slot, lslot = maps
    x, z, zs, e7 = material
    w = R.encode_rows(z * zs, slot)
    zd = R.decode_rows(w, slot)
    scale = R.infer_scale(zd[:-1], z[:-1], "Z")
    assert scale == zs
    R.assert_scale_is(scale, *R.z_scale_arg(e7), what="Z")
    assert R.spectrum_mismatch(zd, z, zs) is None
    # an entry of four words all read as its word 0, for a tone at each sub-position j != 0
    for f in _tone_bins(slot, lslot)[:8]:
        s = int(slot[f])
        if s % 4 == 0:
            continue
        bad = w.copy()
        e0 = s - s % 4
        bad[:, e0:e0 + 4] = bad[:, e0:e0 + 1]
        assert R.spectrum_mismatch(R.decode_rows(bad, slot), z, zs) is not None, f
    # a scale off by two
    with pytest.raises(AssertionError):
        R.assert_scale_is(2.0 * zs, *R.z_scale_arg(e7), what="Z")
    with pytest.raises(AssertionError):
        R.assert_scale_is(0.5 * zs, *R.z_scale_arg(e7), what="Z")
    assert R.spectrum_mismatch(zd * 2.0, z, zs) is not None


def test_low_rows_emulation_is_accepted_and_slot_7n8_rejected(maps, material):
    slot, lslot = maps
    x, z, zs, e7 = material
    low = R.encode_low_rows(z * zs, lslot)
    assert R.low_row_mismatch(low, lslot, z, zs) is None
    bad = low.copy()
    bad[2, lslot[R.LOW_BINS == R.N - R.LOW][0]] = R.words_of_complex(np.array([1.0 + 0.5j]))[0]
    assert R.low_row_mismatch(bad, lslot, z, zs) is not None
    # the miscompile in a low row: an entry holding a tone at j != 0 read as its word 0
    for f in _tone_bins(slot, lslot)[1:8:2]:
        s = int(lslot[np.nonzero(R.LOW_BINS == f)[0][0]])
        if s % 4 == 0:
            continue
        bad = low.copy()
        bad[:, s - s % 4:s - s % 4 + 4] = bad[:, s - s % 4:s - s % 4 + 1]
        assert R.low_row_mismatch(bad, lslot, z, zs) is not None, f


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
def test_pattern_spectra_emulation_is_accepted_and_conjugation_rejected(maps, material, method):
    slot, _ = maps
    x = material[0]
    t = x[1000:1000 + 2 * R.B + 333]
    u = R.pattern_spectra_ref(t, method)
    tn, tn_c, _, _ = R.templ_norms(t)
    ts = R.pow2_under(*R.t_scale_arg(tn_c if method == "ccoeff_normed" else tn)) / R.N
    w = R.encode_rows(u * ts, slot)
    ud = R.decode_rows(w, slot)
    scale = R.infer_scale(ud, u, "U")
    assert scale == ts
    R.assert_scale_is(scale * R.N, *R.t_scale_arg(tn_c if method == "ccoeff_normed" else tn), what="U")
    assert R.spectrum_mismatch(ud, u, ts) is None
    assert R.spectrum_mismatch(np.conj(ud), u, ts) is not None
    # the other method's pattern (centred vs not) is not this one's
    other = R.pattern_spectra_ref(t, "sqdiff_normed" if method == "ccoeff_normed" else "ccoeff_normed")
    assert R.spectrum_mismatch(ud, other, ts) is not None


def _emulate_product(u_w, z_w, g, ms, read_back=None):
    """mac_kernel's product of one pair from stored words (slot order): float32-free emulation -- float64 sums, one rounding to
    halves per pass.  read_back(words) models what a later pass reads of the row it accumulates into."""
    u, z = R.complex_of_words(u_w), R.complex_of_words(z_w)
    partials, mag = R.product_terms(u, z, g)
    y_w = None
    prev = np.zeros(u.shape[1], complex)
    for p in partials:
        chunk = (p - prev) * ms
        prev = p
        base = 0.0 if y_w is None else R.complex_of_words((read_back or (lambda v: v))(y_w[None])[0])
        y_w = R.words_of_complex(base + chunk)
    return y_w, partials, mag


@pytest.fixture(scope="module")
def long_product(maps):
    slot, lslot = maps
    n = 45 * R.B + 1234
    x = _tones(n, _tone_bins(slot, lslot), 2)
    t = _tones(37 * R.B - 100, _tone_bins(slot, lslot)[::-1], 3)
    z = R.block_spectra_ref(x)
    _, e7 = R.stream_stats(x)
    zs = R.pow2_under(*R.z_scale_arg(e7))
    tn = R.templ_norms(t)[0]
    ts = R.pow2_under(*R.t_scale_arg(tn)) / R.N
    ys = R.pow2_under(*R.y_scale_arg(tn, 37, e7))
    ms = ys / (ts * R.N * zs)                          # mac_scale = y_scale / (t_scale z_scale), t_scale = ts N
    return R.encode_rows(R.pattern_spectra_ref(t, "sqdiff_normed") * ts, slot), R.encode_rows(z * zs, slot), ms


def test_products_emulation_is_accepted_and_each_defect_rejected(long_product):
    u_w, z_w, ms = long_product
    u, z = R.complex_of_words(u_w), R.complex_of_words(z_w)
    for g in (0, 1):                                   # pair 1 runs past the stream's end (zero blocks)
        y_w, partials, mag = _emulate_product(u_w, z_w, g, ms)
        assert len(partials) == 2                       # 37 segments: two accumulating passes
        y = R.complex_of_words(y_w)
        assert R.product_mismatch(y, partials, mag, ms) is None
        # the hipcc 7.2 pattern in the accumulating pass: every bin of an entry reads back the first bin's partial sum
        def first_word(v):
            v = v.copy().reshape(-1, 4)
            v[:] = v[:, :1]
            return v.reshape(1, -1)
        bad, _, _ = _emulate_product(u_w, z_w, g, ms, read_back=first_word)
        assert R.product_mismatch(R.complex_of_words(bad), partials, mag, ms) is not None
        # the same on the stored row itself: an entry's four words all its word 0
        bad = y_w.copy().reshape(-1, 4)
        bad[:] = bad[:, :1]
        assert R.product_mismatch(R.complex_of_words(bad.reshape(-1)), partials, mag, ms) is not None
        # one segment left out
        keep = np.ones(u.shape[0], bool)
        keep[5] = False
        short_w, _, _ = _emulate_product(u_w[keep], z_w, g, ms)
        assert R.product_mismatch(R.complex_of_words(short_w), partials, mag, ms) is not None
        # pattern spectra conjugated before the product
        conj_w = R.words_of_complex(np.conj(u))
        cj, _, _ = _emulate_product(conj_w, z_w, g, ms)
        assert R.product_mismatch(R.complex_of_words(cj), partials, mag, ms) is not None
        # a scale off by two
        assert R.product_mismatch(y * 2.0, partials, mag, ms) is not None
        assert R.product_mismatch(y, partials, mag, ms * 2.0) is not None


def test_row_energies_and_half_written_rows(long_product):
    u_w, z_w, ms = long_product
    y_w, _, _ = _emulate_product(u_w, z_w, 0, ms)
    y = R.complex_of_words(y_w)
    e64 = float((np.abs(y) ** 2).sum())
    # the float32 sum as bound_low_kernel forms it (in some order), then its factor: accepted
    e32 = np.float32(0.0)
    for v in (np.abs(y) ** 2).astype(np.float32):
        e32 = np.float32(e32 + v)
    ok, _ = R.energy_ok(float(np.float32(e32 * np.float32(1.000001))), e64, R.N, 1.000001)
    assert ok
    # four times every fourth bin (the hipcc 7.2 energy): rejected on tone material
    wrong = 4.0 * float((np.abs(y[0::4]) ** 2).sum())
    assert not R.energy_ok(wrong * 1.000001, e64, R.N, 1.000001)[0]
    # wave energies: sixteen runs of 1024 words
    we = R.wave_energies(y_w[None])[0]
    assert we.shape == (16,) and abs(we.sum() - e64) <= 1e-9 * e64
    # a half-written row is neither written nor untouched
    rows = np.stack([y_w, np.full_like(y_w, R.NAN_WORD), y_w.copy()])
    rows[2, ::2] = R.NAN_WORD
    assert R.row_states(rows).tolist() == [1, 0, 2]
