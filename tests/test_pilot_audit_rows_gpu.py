"""The band-split form's first pass over the searches (mac_rows_kernel, ROWS_FIRST: a search's pilot row and its audit row from one
read of the pattern's spectra) and the survivors' pass behind it (ROWS_REST: marks scanned first, the audit row not formed again),
against the route they replace (SUSHI_HIP_PILOT_ROWS=list: mac_list_kernel for every pilot, the survivors' pass over every search)
and against float64, on the MI355X.

The job: audio-like material as tests/test_fft_stages_gpu.py's _listed_job has it (180 s of sushi_amd.synth audio at 12 kHz, the
source = the stream advanced by 27,000 samples plus noise; windows of 16 pairs and a ragged end), patterns of 1, 6, 7, 18, 19, 30,
31 and 40 segments -- both instances of mac_rows_kernel, both edges of each and the patterns that stay with mac_list_kernel --, the
last search's window ending with the stream.  One sub-batch (asserted), so that a workspace view covers every pair.

Which whole rows a run wrote is found by the sentinel procedure of the stage tests: fill the Y view with NaN halves, run, fetch the
view.  Under both routes the written rows must be the same rows with the same bits, and every one of them must equal its float64
reference from the stored factors (fft_stage_ref.product_mismatch): the reference, not the other route, says the rows are right.

The audit's hash is the contract tests/test_bound_fault_gpu.py states: run `seq` of a batch audits, of search g, pair
(((g * 2654435761 + seq * 40503) mod 2^32) >> 9) mod n_pairs; with SUSHI_HIP_AUDIT_EVERY=e the searches with (g + seq) % e == 0."""
import functools

import numpy as np
import pytest

import fft_stage_ref as R
import test_fft_stages_gpu as S          # its helpers: material, pair geometry, the product rows' float64 check

pytestmark = pytest.mark.gpu
PAIR = S.PAIR
SEGS = [40, 31, 30, 19, 18, 7, 6, 1]      # the longest first: the last search is short enough for its window to reach the stream's end
ROWS_SMAX = 30                            # patterns of up to this many segments go through mac_rows_kernel


def audit_pair(g, seq, n_pairs):
    return (((g * 2654435761 + seq * 40503) & 0xffffffff) >> 9) % n_pairs


def audited(g, seq, every):
    return every > 0 and (g + seq) % every == 0


@functools.lru_cache(maxsize=None)
def _job(dtype):
    from sushi_amd import synth
    rate, shift = 12000, 27000
    dst_pcm = synth.make_dst_pcm(180, rate, seed=51)
    src_pcm = synth.make_src_pcm(dst_pcm, shift, seed=52)
    dst = S._as(np.clip(dst_pcm.astype(np.float64) / 32768.0 + 0.5, 0, 1), dtype, 1.0)
    src = S._as(np.clip(src_pcm.astype(np.float64) / 32768.0 + 0.5, 0, 1), dtype, 1.0)
    rng = np.random.default_rng(53)
    offs, lens, wst, npos = [], [], [], []
    for k, s in enumerate(SEGS):
        o = 150000 + 230000 * k
        m = s * R.B - 777
        ws = o + shift - int(rng.integers(PAIR, 6 * PAIR))
        p = 16 * PAIR + 123
        if k == len(SEGS) - 1:
            p = dst.shape[0] - m - ws + 1                  # the window ends where the stream ends
        offs.append(o); lens.append(m); wst.append(ws); npos.append(p)
        assert ws >= 0 and ws + p + m - 1 <= dst.shape[0] and o + m <= src.shape[0]
    assert wst[-1] + npos[-1] + lens[-1] - 1 == dst.shape[0]
    for a in (dst, src):
        a.setflags(write=False)
    return dst, src, offs, lens, wst, npos


@functools.lru_cache(maxsize=None)
def _streams(dtype):
    """the two device streams and the stream's stored spectra as complex128, made once per sample type"""
    from sushi_amd.device import DeviceStream
    job = _job(dtype)
    D, Sx = DeviceStream(job[0]), DeviceStream(job[1])
    z_c = R.complex_of_words(R.words(D.spectra(), R.N))
    z_c.setflags(write=False)
    return D, Sx, z_c


@functools.lru_cache(maxsize=None)
def _oracle_index(dtype, method):
    from oracle import oracle as O
    O.build()
    rows = S._oracle_rows(O, _job(dtype), method)
    return [int(np.argmax(r) if method == "ccoeff_normed" else np.argmin(r)) for r in rows]       # (the first extremum)


def _batch(dtype, method, exclusion):
    from sushi_amd.device import SearchBatch
    D, Sx, _ = _streams(dtype)
    _, _, offs, lens, wst, npos = _job(dtype)
    b = SearchBatch(D, Sx, offs, lens, wst, npos, path="fft", method=method, exclusion=exclusion)
    return b


def _result(b):
    idx, score = b.results()
    return idx.astype(np.int64).tolist(), score.copy().view(np.uint32).tolist()


def _geometry(lib, dtype):
    """[(first pair in the batch, pairs, segments)] per search"""
    _, _, offs, lens, wst, npos = _job(dtype)
    out, pr0 = [], 0
    for w, p, m in zip(wst, npos, lens):
        _, n_pairs, n_seg = S._pairs_of(lib, w, p, m)
        out.append((pr0, n_pairs, n_seg))
        pr0 += n_pairs
    return out


def _sentinel_runs(b, runs):
    """Run once (run 0 of the batch), then `runs` times: fill the Y view with the sentinel, run, fetch the view.  -> per sentinel
    run (its number, result, diagnostics, written[pairs], the Y words); never a half-written row."""
    import torch
    from sushi_amd import _native
    b.run()
    assert b.sub_batches == 1
    out = []
    for seq in range(1, 1 + runs):
        yv = b.workspace_view(_native.WS_Y)
        ptr = yv.data_ptr()
        yv.view(torch.int32).fill_(R.NAN_WORD)
        b.run()
        yv2 = b.workspace_view(_native.WS_Y)
        assert yv2.data_ptr() == ptr and yv2.numel() == yv.numel()
        d = b.diagnostics()
        assert d["band"] == 1
        yw = R.words(yv2, R.N)
        st = R.row_states(yw)
        assert (st != 2).all(), np.nonzero(st == 2)[0]
        written = st == 1
        assert written.sum() >= d["pairs_transformed"], (written.sum(), d["pairs_transformed"])
        out.append((seq, _result(b), d, written, yw))
    return out


def _check_rows(geo, lib, job, yw, z_c, u_c, written, scales, what):
    """Every written row against mac_scale * sum_s conj(U_s) Z_{6g+s} of the stored factors in float64 (R.product_mismatch: its
    allowance counts a rounding per accumulating pass).  mac_scale is the host's own power of two per search (the stage tests
    show the device's equal to it); it is not inferred from the rows here: the largest bin of a row of two passes may be further
    from its reference than one rounding to a half, which is what R.infer_scale allows."""
    _, _, offs, lens, wst, npos = job
    checked, s0 = 0, 0
    for g, (p0, n_pairs, n_seg) in enumerate(geo):
        pair0 = S._pairs_of(lib, wst[g], npos[g], lens[g])[0]
        for i in np.flatnonzero(written[p0:p0 + n_pairs]):
            partials, mag = R.product_terms(u_c[s0:s0 + n_seg], z_c, pair0 + int(i))
            bad = R.product_mismatch(R.complex_of_words(yw[p0 + i]), partials, mag, scales[g])
            assert bad is None, (what, g, n_seg, int(i), bad)
            checked += 1
        s0 += n_seg
    return checked


@pytest.fixture(scope="module")
def lib():
    from sushi_amd import _native
    L = _native.lib()
    assert (L.sushi_hip_fft_size(), L.sushi_hip_fft_block()) == (R.N, R.B)
    return L


def test_the_job_crosses_every_route(lib):
    geo = _geometry(lib, "u8")
    assert [s for _, _, s in geo] == SEGS
    assert all(n >= 16 for _, n, _ in geo)
    # every first-pass row lies inside its search, and at audit rate 2 both parities of the run number audit somebody
    for every, seqs in ((1, (1,)), (2, (1, 2))):
        for seq in seqs:
            assert any(audited(g, seq, every) for g in range(len(SEGS)))
    # the run the bound-fault check takes exists early on (a total fault makes pair 0 every pilot)
    assert _fault_run(geo) < 8


def _fault_run(geo):
    """the first run in which no search's audit pair is its pair 0"""
    return next(seq for seq in range(64) if all(audit_pair(g, seq, n) != 0 for g, (_, n, _) in enumerate(geo)))


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("every", [1, 2])
def test_first_pass_rows_are_the_list_routes_rows_and_the_references(lib, monkeypatch, method, dtype, every):
    """Index and score bits equal the run without exclusion and the oracle's index; under both routes the same rows are written with
    the same bits; every written row equals its float64 reference; at audit rate 1 no audit is lost or doubled.  (The one row the
    first pass can add is an audit pair's that the first bound keeps and the second look then drops: the list route never forms
    it.  The runs taken here hold no such pair; the test prints the rows that differ before it asserts that there are none.)"""
    from sushi_amd import _native
    job = _job(dtype)
    geo = _geometry(lib, dtype)
    z_c = _streams(dtype)[2]
    scales = S._host_mac_scales(job, method)
    monkeypatch.delenv("SUSHI_HIP_TEST_BOUND_FAULT", raising=False)
    monkeypatch.delenv("SUSHI_HIP_PILOT_ROWS", raising=False)
    never = _batch(dtype, method, "never")
    never.run()
    want = _result(never)
    assert want[0] == _oracle_index(dtype, method)
    monkeypatch.setenv("SUSHI_HIP_AUDIT_EVERY", str(every))
    runs = 1 if every == 1 else 2                                     # (rate 2: both parities of the run number)
    got = {}
    for route in ("default", "list"):
        if route == "list":
            monkeypatch.setenv("SUSHI_HIP_PILOT_ROWS", "list")
        b = _batch(dtype, method, "band")
        got[route] = _sentinel_runs(b, runs)
        if route == "default":
            # every written row against float64, from the stored pattern spectra of this batch
            u_c = R.complex_of_words(R.words(b.workspace_view(_native.WS_TSPEC), R.N))
            for seq, res, d, written, yw in got[route]:
                assert _check_rows(geo, lib, job, yw, z_c, u_c, written, scales, "Y rows, run %d" % seq) == written.sum()
    report = []
    for (seq, res, d, written, yw), (seq_l, res_l, d_l, written_l, yw_l) in zip(got["default"], got["list"]):
        assert seq == seq_l
        assert res == want and res_l == want, (seq, res[0], res_l[0], want[0])
        assert d["slb_violations"] == 0 and d["flagged"] == 0 and d_l["slb_violations"] == 0, (d, d_l)
        # the first pass's rows exist: the pilot's, and the audit pair's of every audited search that mac_rows_kernel takes
        first_pass = 0
        for g, (p0, n_pairs, n_seg) in enumerate(geo):
            assert written[p0:p0 + n_pairs].any(), (seq, g)
            if n_seg <= ROWS_SMAX and audited(g, seq, every):
                assert written[p0 + audit_pair(g, seq, n_pairs)], (seq, g, audit_pair(g, seq, n_pairs))
                first_pass += 1
        assert first_pass >= (6 if every == 1 else 3), (seq, first_pass)
        assert not written.all() and d["pairs_transformed"] < b.fft_pairs              # (the bound excludes: rows are left untouched)
        extra, missing = np.flatnonzero(written & ~written_l), np.flatnonzero(written_l & ~written)
        print("\npilot/audit rows %s %s every %d run %d: rows written %d (list route %d; only here %s, only there %s), pairs_transformed %d / %d, "
              "excluded_audited %d / %d" % (method, dtype, every, seq, int(written.sum()), int(written_l.sum()), extra.tolist(), missing.tolist(),
                                            d["pairs_transformed"], d_l["pairs_transformed"], d["excluded_audited"], d_l["excluded_audited"]))
        report.append((extra, missing))
        assert d["pairs_transformed"] == d_l["pairs_transformed"], (seq, d, d_l)
        if every == 1:
            assert d["excluded_audited"] == d_l["excluded_audited"] and d["excluded_audited"] > 0, (seq, d, d_l)
        both = written & written_l
        assert (yw[both] == yw_l[both]).all(), (seq, np.flatnonzero((yw[both] != yw_l[both]).any(axis=1)))
    for extra, missing in report:
        assert extra.size == 0 and missing.size == 0, (extra.tolist(), missing.tolist())       # the same rows under both routes


@pytest.mark.parametrize("method", ["sqdiff_normed", "ccoeff_normed"])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_a_wrong_bound_is_caught_by_the_first_pass_audit_row(lib, monkeypatch, method, dtype):
    """SUSHI_HIP_TEST_BOUND_FAULT=1:0: every stored bound of every search reads +inf, so pair 0 is every pilot and every other pair
    is excluded; the audit pair -- formed in the first pass -- is what shows the bound wrong, and the run ends with the oracle's
    results all the same.  (The variable only overwrites stored bounds.)"""
    geo = _geometry(lib, dtype)
    monkeypatch.delenv("SUSHI_HIP_TEST_BOUND_FAULT", raising=False)
    monkeypatch.delenv("SUSHI_HIP_PILOT_ROWS", raising=False)
    never = _batch(dtype, method, "never")
    never.run()
    want = _result(never)
    assert want[0] == _oracle_index(dtype, method)
    monkeypatch.setenv("SUSHI_HIP_AUDIT_EVERY", "1")
    monkeypatch.setenv("SUSHI_HIP_TEST_BOUND_FAULT", "1:0")
    b = _batch(dtype, method, "band")
    assert b.sub_batches == 1
    last = _fault_run(geo)
    for seq in range(last + 1):
        b.run()
        if all(audit_pair(g, seq, n) != 0 for g, (_, n, _) in enumerate(geo)):
            assert _result(b) == want, seq
    d = b.diagnostics()
    assert d["band"] == 1 and d["excluded_audited"] > 0 and d["slb_violations"] > 0, d      # (the fault bit, and the audit saw it)
