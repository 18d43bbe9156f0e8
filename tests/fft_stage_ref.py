"""Float64 references of the FFT path's stages and the comparators that hold the GPU's stored halves to them (a helper of
tests/test_fft_stages_gpu.py and tests/test_fft_stage_ref.py; plain NumPy, no GPU, nothing of the product's arithmetic).

What each stage stores (sushi_fft_spectra.inc, sushi_fft_store.inc, mac_core.hpp, sushi_fft_mac.inc):

* block spectra   Z_j = z_scale * DFT_N(xc[jB .. jB+N) + i xc[jB+H .. jB+H+N)),  xc = x - c,  c = float32(mean x),
                  zeros past the end of the stream, one all-zero block behind the last;
* low rows        the bins |f| < N/8 of the same row (the same halves), slot 7N/8 zero;
* rest norms      [0] |Z| over the bins outside the band, [1] / [2] the same of the two real blocks Z packs,
                  A = (Z(f) + conj Z(N-f)) / 2, B = (Z(f) - conj Z(N-f)) / 2i -- each of the halves AS STORED;
* pattern spectra U_s = (t_scale / N) * DFT_N(t_s),  t_s = segment s of the pattern (B samples, zero padded); the pattern as
                  it is for sqdiff_normed, minus float32(its mean) for ccoeff_normed (tspec_kernel);
* products        Y_g = mac_scale * sum_s conj(U_s) * Z_{STEP g + s},  g the ABSOLUTE pair index.

THE CONJUGATION.  tspec_kernel stores the forward transform of the segment itself (the comment above it: Tt = conj(DFT(t_s)) / N
"stored as the packed halves (Re Tt, -Im Tt) ... the scaled forward transform itself"), and mac_core.hpp forms
Re = dot2(U, Z), Im = dot2(U, -i Z) = Re(conj(U) Z), Im(conj(U) Z).  So the products are conj(U) * Z of the halves as stored.

Every stored spectrum is one 32-bit word per bin (re | im << 16, two IEEE halves), in the order the inverse transform loads
them (sushi_hip_fft_slot_of_bin) or, for low rows, the order bound_low_kernel loads them (sushi_hip_fft_low_slot_of_bin).
A product is elementwise, so references of products are formed slot by slot and need no map.
"""
import math

import numpy as np

N, B = 16384, 4096
H = N - B
STEP = 6
SMAX_LONG = 30                      # mac_long_kernel / mac_list_kernel: segments per accumulating pass
LOW = N // 8                        # the band: |f| < N/8
LOW_WORDS = N // 4                  # words of a low row
U11 = 2.0 ** -11                    # a half's rounding, relative
U24 = 2.0 ** -24                    # a float32 rounding, relative
SUB = 2.0 ** -25                    # a half's rounding below its normal range (subnormal spacing 2^-24), absolute
E_F = 1e-5                          # the float32 forward transforms' error in the 2-norm, relative (Higham Thm 24.2)
NAN_WORD = 0x7E007E00               # two quiet-NaN halves: the sentinel of a row no kernel wrote

LOW_BINS = np.concatenate([np.arange(LOW), np.arange(N - LOW, N)])     # the 4096 bins a low row has a slot for


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-24: the relative error of n float32 roundings in a chain (Higham 3.1)."""
    return n * U24 / (1.0 - n * U24)


# --------------------------------------------------------------------------------------------------- slot maps, decoding

def slot_maps(lib):
    """(slot[f] of a whole row, lslot[i] of LOW_BINS[i] in a low row) from the library's host-only exports."""
    slot = np.array([lib.sushi_hip_fft_slot_of_bin(f) for f in range(N)], np.int64)
    lslot = np.array([lib.sushi_hip_fft_low_slot_of_bin(int(f)) for f in LOW_BINS], np.int64)
    assert sorted(slot.tolist()) == list(range(N)) and sorted(lslot.tolist()) == list(range(LOW_WORDS))
    return slot, lslot


def words(view, row_words):
    """A float16 view of packed halves (torch tensor or ndarray) -> uint32 words [rows][row_words]."""
    a = view.cpu().numpy() if hasattr(view, "cpu") else np.asarray(view)
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, row_words)


def complex_of_words(w):
    """uint32 words (re | im << 16) -> complex128, element by element (the stored order kept)."""
    h = np.ascontiguousarray(w, dtype=np.uint32).view(np.uint16).reshape(w.shape + (2,)).view(np.float16).astype(np.float64)
    return h[..., 0] + 1j * h[..., 1]


def words_of_complex(z):
    """complex values -> words, each part rounded to the nearest half (ties to even: v_cvt_pk_f16_f32, pack_h2), never infinite."""
    re = np.clip(z.real, -65504.0, 65504.0).astype(np.float16).view(np.uint16).astype(np.uint32)
    im = np.clip(z.imag, -65504.0, 65504.0).astype(np.float16).view(np.uint16).astype(np.uint32)
    return re | (im << 16)


def decode_rows(w, slot):
    """Whole rows: words in the load order -> complex rows in natural bin order."""
    return complex_of_words(w)[:, slot]


def decode_low_rows(w, lslot):
    """Low rows -> complex [rows][N] in natural bin order, zero outside LOW_BINS."""
    out = np.zeros((w.shape[0], N), complex)
    out[:, LOW_BINS] = complex_of_words(w)[:, lslot]
    return out


def encode_rows(z, slot):
    """Natural-order complex rows -> stored words (the emulation of a kernel's store)."""
    w = np.zeros(z.shape, np.uint32)
    w[:, slot] = words_of_complex(z)
    return w


def encode_low_rows(z, lslot):
    w = np.zeros((z.shape[0], LOW_WORDS), np.uint32)
    w[:, lslot] = words_of_complex(z[:, LOW_BINS])
    w[:, lslot[LOW_BINS == N - LOW]] = 0
    return w


# --------------------------------------------------------------------------------------------------- scales (sushi_fft_store.inc)

def _pow2_exponent(target, bound):
    return None if not bound > 0 else float(np.clip(math.floor(math.log2(target / bound)), -60, 60))


def _pow2_arg(target, bound):
    return math.log2(target / bound) if bound > 0 else None


def z_scale_arg(e7):
    return 32768.0, 181.02 * math.sqrt(e7)


def t_scale_arg(tnorm):
    return 8192.0, 64.0 * tnorm / N


def y_scale_arg(tnorm, n_seg, e7):
    return 32768.0, (64.0 * math.sqrt(n_seg) * tnorm / N) * (169.33 * math.sqrt(e7))


def pow2_under(target, bound):
    k = _pow2_exponent(target, bound)
    return 1.0 if k is None else 2.0 ** k


def stream_stats(x):
    """(c, E7) of a stream (fft_stats_kernel): c = float32 of the mean, E7 = the largest centred energy of STEP + 1 consecutive
    blocks (the last ones clipped at the stream's end)."""
    x64 = np.asarray(x, np.float64)
    n = x64.shape[0]
    c = float(np.float32(x64.sum() / n))
    nb = -(-n // B)
    e = np.zeros(nb * B)
    e[:n] = (x64 - c) ** 2
    eb = e.reshape(nb, B).sum(axis=1)
    cs = np.concatenate([[0.0], np.cumsum(eb)])
    e7 = max(cs[min(j + STEP + 1, nb)] - cs[j] for j in range(nb))
    return c, float(e7)


def templ_norms(t):
    """(|T|, |T - mean T|, float32(mean T)) as tspec_kernel takes them (templ_stats: cv2's order of operations)."""
    t64 = np.asarray(t, np.float64)
    m = t64.shape[0]
    mean = t64.sum() / m
    var = max((t64 * t64).sum() / m - mean * mean, 0.0)
    return math.sqrt(var + mean * mean) * math.sqrt(m), math.sqrt(var) * math.sqrt(m), float(np.float32(mean)), var < 2.220446049250313e-16


def infer_scale(stored, ref, what):
    """The power of two `stored` carries over `ref` (rows that are not all zero), asserted one value and a power of two:
    |log2 ratio - round| < 1e-3 (a half holds 11 bits: the largest bin of a row is within 2^-11 of its own size)."""
    stored, ref = np.atleast_2d(stored), np.atleast_2d(ref)
    ks = []
    for r in range(ref.shape[0]):
        mr = np.abs(ref[r]).max()
        if mr == 0.0:
            assert not np.abs(stored[r]).any(), "%s: row %d should be zero" % (what, r)
            continue
        k = math.log2(np.abs(stored[r]).max() / mr)
        assert abs(k - round(k)) < 1e-3, "%s: row %d's scale 2^%.6f is not a power of two" % (what, r, k)
        ks.append(int(round(k)))
    assert len(set(ks)) <= 1, "%s: more than one scale %s" % (what, sorted(set(ks)))
    return 2.0 ** ks[0] if ks else None


def assert_scale_is(observed, target, bound, what):
    """The inferred power of two equals the host's pow2_under(target, bound) -- the neighbouring one only where the host's argument
    log2(target / bound) lies within 1e-6 of an integer (the device computes it in its own order)."""
    if observed is None:
        return
    want = pow2_under(target, bound)
    if observed == want:
        return
    arg = _pow2_arg(target, bound)
    near = arg is not None and abs(arg - round(arg)) < 1e-6 and observed in (want * 2.0, want / 2.0)
    assert near, "%s: scale %r, the host's restatement says %r (log2 argument %r)" % (what, observed, want, arg)


# --------------------------------------------------------------------------------------------------- float64 references

def block_spectra_ref(x):
    """Z_j (unscaled) for every block j of the stream plus the all-zero one behind it: [ceil(n / B) + 1][N] complex."""
    x64 = np.asarray(x, np.float64)
    n = x64.shape[0]
    c, _ = stream_stats(x)
    nb = -(-n // B)
    xc = np.zeros((nb + 1) * B + H + N)
    xc[:n] = x64 - c
    rows = [np.fft.fft(xc[j * B:j * B + N] + 1j * xc[j * B + H:j * B + H + N]) for j in range(nb)]
    return np.array(rows + [np.zeros(N, complex)])


def rest_bins():
    """The bins outside the band, with 7N/8 (the band is |f| < N/8 strictly: mirror-symmetric)."""
    r = np.setdiff1d(np.arange(N), LOW_BINS[LOW_BINS != N - LOW])
    assert sorted(((-r) % N).tolist()) == sorted(r.tolist())
    return r


def rest_norms64(z_stored):
    """float64 norms outside the band of stored rows (natural order): of Z, of its real block A, of its real block B."""
    r = rest_bins()
    zm = np.conj(z_stored[:, (-np.arange(N)) % N])
    zn = np.sqrt((np.abs(z_stored[:, r]) ** 2).sum(axis=1))
    an = np.sqrt((np.abs((z_stored + zm)[:, r] / 2) ** 2).sum(axis=1))
    bn = np.sqrt((np.abs((z_stored - zm)[:, r] / 2) ** 2).sum(axis=1))
    return zn, an, bn


def pattern_spectra_ref(t, method):
    """U_s (unscaled: DFT_N of segment s) of one pattern: [ceil(M / B)][N] complex."""
    t64 = np.asarray(t, np.float64)
    m = t64.shape[0]
    if method == "ccoeff_normed":
        t64 = t64 - templ_norms(t)[2]
    n_seg = -(-m // B)
    rows = []
    for s in range(n_seg):
        seg = np.zeros(N)
        piece = t64[s * B:(s + 1) * B]
        seg[:piece.shape[0]] = piece
        rows.append(np.fft.fft(seg))
    return np.array(rows)


def product_terms(u, z, pair_abs):
    """The float64 partial sums of one product row, pass by pass, from STORED factors in any common order of slots:
    (partials[c] = sum over the segments of passes 0 .. c of conj(U_s) * Z_{STEP g + s}, sum_s |U_s| |Z_{STEP g + s}|).
    Blocks past the stream (index >= rows of z - 1, the all-zero row) are zero."""
    n_seg = u.shape[0]
    zero = z.shape[0] - 1
    acc = np.zeros(u.shape[1], complex)
    mag = np.zeros(u.shape[1])
    partials = []
    for s in range(n_seg):
        j = STEP * pair_abs + s
        zj = z[j] if j < zero else 0.0 * z[zero]
        acc = acc + np.conj(u[s]) * zj
        mag = mag + np.abs(u[s]) * np.abs(zj)
        if (s + 1) % SMAX_LONG == 0 or s == n_seg - 1:
            partials.append(acc.copy())
    return partials, mag


# --------------------------------------------------------------------------------------------------- comparators

def _worst(d, tol):
    bad = d > tol
    if not bad.any():
        return None
    i = np.unravel_index(int(np.argmax(np.where(bad, d / np.maximum(tol, 1e-300), 0))), d.shape)
    return i, float(d[i]), float(tol[i])


def spectrum_mismatch(stored, ref, scale):
    """Where stored rows (natural order, complex of the stored halves) differ from scale * ref by more than the stage may:

    per component p (re, im) of every bin, |stored/scale - ref|_p <= (2^-11 + 2^-24) |ref_p| + (1 + 2^-11) e |ref|_2 + 2^-25 / scale
      * 2^-11 |ref_p|     -- the one rounding to a half (round to nearest: half an ulp of 11 bits), of the component's own size;
      * e |ref|_2          -- the float32 forward transform, e = E_F + 2 u: Higham's 2-norm bound (DESIGN.md 3.3, 1e-5 for 14
                              radix-2 levels with twiddles good to 4 u) plus the float32 centring / mean subtraction of the input
                              (u |x - c| per sample: u |ref|_2 by Parseval) and the product by the power of two; an error of 2-norm
                              e |ref|_2 is at most that in any one component; the half's rounding acts on it too (the 2^-11 factor);
      * 2^-24 |ref_p|     -- the float32 product by the scale factor t_scale / N or z_scale (exact unless subnormal: kept as a u);
      * 2^-25 / scale     -- the half format's subnormal floor: below 2^-14 the spacing is 2^-24, half of it absolute.
    Returns None, or (index, |difference|, allowance) of the worst component."""
    stored, ref = np.atleast_2d(stored), np.atleast_2d(ref)
    nrm = np.sqrt((np.abs(ref) ** 2).sum(axis=1, keepdims=True))
    e = E_F + 2 * U24
    out = None
    for part in (np.real, np.imag):
        d = np.abs(part(stored) / scale - part(ref))
        tol = (U11 + U24) * np.abs(part(ref)) + (1 + U11) * e * nrm + SUB / scale
        out = out or _worst(d, tol)
    return out


def product_mismatch(stored, partials, mag, mac_scale):
    """Where a stored product row (slot order, complex of its halves) differs from mac_scale * sum_s conj(U_s) Z_s of the STORED
    factors by more than mac_kernel / mac_long_kernel / mac_list_kernel / mac_rows_kernel may:

    per component p, |stored/mac_scale - ref|_p <= (1 + 2^-10) [ sum_c (2^-11 + 2^-23) |P_c|_p + gamma_62 sum_s |U_s| |Z_s| ]
                                                  + passes 2^-25 / mac_scale
      * P_c: the float64 partial sum after accumulating pass c (30 segments a pass; one pass for up to 30 segments); every pass
        ends in one rounding to a half of what has been accumulated so far (2^-11 of it), after a float32 product by mac_scale
        and -- passes after the first -- a float32 addition of the half read back (2^-24 each: the 2^-23);
      * gamma_62 sum_s |U_s||Z_s|: the float32 v_dot2 accumulation of a pass: at most 30 dot2 (the classes pad 6 / 12 / 18 / 24 / 30
        with zero segments, which add exactly nothing), each two products of halves (exact in float32) added with at most two
        roundings: 60 roundings, plus the product by mac_scale and the pass's addition.  |Re(conj(U) Z)| terms: |a c| + |b d|
        <= |U||Z| (Cauchy-Schwarz), the same for the imaginary part.  Earlier passes' errors are carried in the half that is
        read back: their sum is what the (1 + 2^-10) covers beyond first order;
      * 2^-25 / mac_scale: the half format's subnormal floor, once a pass.
    Returns None, or (index, |difference|, allowance) of the worst component."""
    passes = len(partials)
    ref = partials[-1]
    out = None
    for part in (np.real, np.imag):
        d = np.abs(part(stored) / mac_scale - part(ref))
        tol = sum((U11 + 2 * U24) * np.abs(part(p)) for p in partials) + gamma(62) * mag
        tol = (1 + 2.0 ** -10) * tol + passes * SUB / mac_scale
        out = out or _worst(d, tol)
    return out


def energy_ok(acc, stored_energy64, n_adds, factor):
    """A float32 sum of squares of halves as the kernel forms it (products of halves are exact in float32; every term >= 0, so
    n chained roundings err by at most gamma_n of the sum), times the kernel's own `factor` (one rounding more):
    factor (1 - gamma_{n+1}) E <= acc <= factor (1 + gamma_{n+1}) E."""
    g = gamma(n_adds + 1)
    lo, hi = factor * stored_energy64 * (1 - g), factor * stored_energy64 * (1 + g)
    return lo <= acc <= hi, (lo, hi)


def wave_energies(y_words):
    """bound_kernel's NEED_Q energy of a whole row: wave n1 (of 16) loads the entries wslot_uint4(64 n1 + lane, u) =
    256 n1 + 64 u + lane, u < 4, lane < 64 -- the 1024 consecutive stored words from 1024 n1 on; its sum of |re|^2 + |im|^2
    (add_abs2_entry), float64, of every wave.  acc[1] is the largest (atomicMax)."""
    y = complex_of_words(y_words)
    return (np.abs(y) ** 2).reshape(y.shape[0], 16, N // 16).sum(axis=2)


def low_cross_term_max(y_low_natural):
    """The signed low-band part of a pair's cross term, per row, in the stored units of Y: y[r] = sum over the band of Y(f) w^(f r),
    every r of the N-point grid (the pair's first half reads real parts, its second half imaginary parts).  bound_low_kernel's
    acc[0] bounds both from above (the low band at its N/2 sample points, sqrt(2) for the points between: a trigonometric
    polynomial of degree < N/8 sampled at N/2 points exceeds its samples by at most sec(pi/4); bin 0 added signed).  The max
    over all r of Re and Im does not depend on the sign convention of the transform (r -> -r)."""
    y = np.fft.ifft(y_low_natural, axis=1) * N
    return np.maximum(y.real.max(axis=1), y.imag.max(axis=1))


def cross_term_modulus_max(y_natural):
    """The cross term's modulus of whole rows: max over r of |sum_f Y(f) w^(f r)| (what bound_kernel's acc[0] bounds)."""
    return np.abs(np.fft.ifft(y_natural, axis=1) * N).max(axis=1)


def low_row_mismatch(low_words, lslot, ref, scale):
    """Low rows (words as stored) against the reference of their whole rows: slot 7N/8 must be exactly zero (the band is
    mirror-symmetric: that bin is counted with the rest), every other bin of the band as spectrum_mismatch.  None, or a description."""
    z7 = low_words[:, lslot[LOW_BINS == N - LOW][0]]
    if z7.any():
        return "slot 7N/8 is not zero in rows %s" % np.nonzero(z7)[0].tolist()
    z = complex_of_words(low_words)[:, lslot]
    keep = LOW_BINS != N - LOW
    return spectrum_mismatch(z[:, keep], np.atleast_2d(ref)[:, LOW_BINS[keep]], scale)


def row_states(w):
    """Per row of words: 0 = every word the NaN sentinel (not written), 1 = no word the sentinel (written), 2 = a mix."""
    s = (w == NAN_WORD).sum(axis=1)
    return np.where(s == w.shape[1], 0, np.where(s == 0, 1, 2))
