"""SearchBatch, the stateful object of the search path, away from its one everyday calling pattern (run() on the current stream,
results() at once): runs on a stream of the caller's, runs nobody collected, a batch re-planned under a pending run.

Two devices serve every test here.
  * A FILLER: matrix products on tensors made beforehand, enqueued on the stream under test AHEAD of the batch's work, so that the
    host calls that follow return while the GPU is still busy with it.  Its length is measured, once per module run: one product
    is timed with events, `reset` + `run` of a drop-in sized batch with the host's clock, and the product is repeated until the
    filler lasts 100 times that host time (a busy host must not void the premise) and at least 20 ms -- ten times the 2 ms
    results() polls its early records for before it falls back on the stream: a read that waits for the wrong stream must still
    find the filler running.  More than one second of filler fails the test.  Where a test relies on work being pending it says
    so: `stream.query()` is False right after the host calls.
  * POISON: every buffer a run can answer through holds -7 before the run is issued, so that a read that came too soon is
    visibly wrong and not, by accident, an earlier run's identical answer.

Inputs: the material of test_gpu_parity.test_early_records_hold_the_answer_or_say_flagged -- a 240,000-sample stream whose second
half is noise, patterns of 4097 .. 9000 samples cut from that half (an exact copy each: the answer is tmpl_off - win_start, and
unique), windows of 50 .. 60 k positions, none flagged -- as float32 and as a uint8 twin whose sums are integers, so that the
oracle's argmin and float32 score are the batch's bit for bit.  Set B is set A with every window moved by one block pair (6 * 4096
samples: the same plan geometry) and every planted copy at another offset: all answers differ, and a run that takes the other
set's descriptors -- what test 5 is there to catch -- computes that set's answer and nothing worse.  The lanes-sized batch is
test_pair_exclusion's 64-event job under SUSHI_HIP_LANES=4:2 with 0.6 of the one-sub-batch workspace; its reference bits come from
a 1:1 batch on the current stream."""
import math
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIR = 6 * 4096
LENS = [9000, 4097, 6000, 9000, 4097, 7001]
NPOS = [60000, 50001, 55000, 52000, 50000, 58000]
WST = {"A": [130000, 160000, 121000, 140000, 150000, 125000]}
WST["B"] = [w + PAIR for w in WST["A"]]
ANSWER = {"A": [20000, 30000, 14000, 40000, 45000, 35000], "B": [43000, 25500, 19000, 11345, 37000, 7000]}
# (as test_native_abi builds them: more pairs and segments than a batch made for the sets above, without headroom, has room for)
TOO_LARGE = ([0, 1000, 2000], [48000] * 3, [0, 100, 200], [190000] * 3)
METHODS = ["sqdiff_normed", "ccoeff_normed"]
FILLER_FLOOR_S = 20e-3
# What a drop-in call's batch gets outside this suite, whose conftest asks for the exclusion 'always': in AUTO a batch this small
# leaves the exclusion out, and with it the ONE synchronisation a run may make (the first run of a batch that goes through the
# exclusion in AUTO or ALWAYS reads 8 bytes back to choose its form) -- a run that waits for its own stream has waited for the
# filler too, and nothing is left pending for a test to catch.
DROP_IN = {"exclusion": "auto"}


def _requests(which, n):
    wst, ans = WST[which][:n], ANSWER[which][:n]
    return [w + a for w, a in zip(wst, ans)], LENS[:n], wst, NPOS[:n]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    return (got[0] == want[0]).all() and (_bits(got[1]) == _bits(want[1])).all()


def _poison(b):
    import torch
    b.out_idx.fill_(-7)
    b.out_score.fill_(-7.0)
    if b._packed is not None:
        b._packed.fill_(-7)
    if b._host_rec is not None:
        b._host_rec.fill_(-7)
    if b._early is not None:
        b._early[:, :2] = -7
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def rows():
    rng = np.random.default_rng(5)
    t = np.arange(120000, dtype=np.float64)
    smooth = (0.5 + 0.3 * np.sin(2 * np.pi * t / 5000.0)).astype(np.float32)
    noisy = (rng.standard_normal(120000) * 0.2 + 0.5).clip(0, 1).astype(np.float32)
    img = np.concatenate([smooth, noisy])
    assert img.shape[0] == 240000 and max(w + p + m - 1 for w, p, m in zip(WST["B"], NPOS, LENS)) <= 240000
    return {"float32": img, "uint8": np.round(img * 255.0).astype(np.uint8)}


@pytest.fixture(scope="module")
def devs(rows):
    from sushi_amd.device import DeviceStream
    return {k: DeviceStream(v) for k, v in rows.items()}


@pytest.fixture(scope="module")
def reference(devs):
    """(idx, score) of a fresh batch's run on the current stream, collected at once -- computed once per case, never changed."""
    import torch
    from sushi_amd.device import SearchBatch
    cache = {}

    def get(dtype, which, n, path="fft", method="sqdiff_normed"):
        key = (dtype, which, n, path, method)
        if key not in cache:
            b = SearchBatch(devs[dtype], devs[dtype], *_requests(which, n), path=path, method=method, **DROP_IN)
            b.run()
            idx, score = b.results()
            torch.cuda.synchronize()
            assert list(idx) == ANSWER[which][:n], (key, idx)          # the planted copies, every one
            if b._early is not None:
                assert not b._early.numpy()[:, 3].any()                # none flagged: the early records are the answer
            idx, score = idx.copy(), score.copy()
            idx.setflags(write=False); score.setflags(write=False)
            cache[key] = (idx, score)
        return cache[key]
    return get


@pytest.fixture(scope="module")
def side():
    import torch
    return torch.cuda.Stream()


class _Filler(object):
    SIZE = 4096

    def __init__(self, host_s, streams):
        import torch
        self.a = torch.rand((self.SIZE, self.SIZE), device="cuda")
        self.c = torch.empty_like(self.a)
        for s in streams:                                  # (the product's first use of a stream may allocate: not inside a test)
            self._enqueue(s, 1)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        self._enqueue(torch.cuda.current_stream(), 1)
        e1.record()
        torch.cuda.synchronize()
        self.unit_s = e0.elapsed_time(e1) * 1e-3
        self.host_s = host_s
        self.repeats = int(math.ceil(max(100.0 * host_s, FILLER_FLOOR_S) / self.unit_s))

    def _enqueue(self, stream, count):
        import torch
        with torch.cuda.stream(stream):
            for _ in range(count):
                torch.mm(self.a, self.a, out=self.c)

    def __call__(self, stream):
        assert self.repeats * self.unit_s <= 1.0, (self.repeats, self.unit_s, self.host_s)
        self._enqueue(stream, self.repeats)


@pytest.fixture(scope="module")
def filler(devs, side):
    import torch
    from sushi_amd.device import SearchBatch
    b = SearchBatch(devs["float32"], devs["float32"], *_requests("A", 3), path="fft", headroom=4.0, **DROP_IN)
    b.run(); b.results()
    torch.cuda.synchronize()
    times = []
    for r in range(6):
        t0 = time.perf_counter()
        assert b.reset(*_requests("AB"[(r + 1) % 2], 3))
        b.run()
        times.append(time.perf_counter() - t0)
        b.results()
        torch.cuda.synchronize()
    f = _Filler(float(np.median(times[1:])), [torch.cuda.current_stream(), side])
    print("filler: unit %.3f ms, reset + run %.1f us, %d repeats" % (f.unit_s * 1e3, f.host_s * 1e6, f.repeats))
    return f


# ---- A. a run on a caller's stream gives the current-stream bits and is waited for ----

WAYS = [(3, "fft", "sqdiff_normed", True), (3, "fft", "ccoeff_normed", True), (3, "direct", "sqdiff_normed", True),
        (6, "fft", "sqdiff_normed", True), (6, "fft", "sqdiff_normed", False)]


@pytest.mark.parametrize("dtype", ["float32", "uint8"])
@pytest.mark.parametrize("n,path,method,packed", WAYS, ids=["early", "early-ccoeff", "host-records", "packed", "out-tensors"])
def test_results_wait_for_the_stream_the_run_was_given(oracle, rows, devs, reference, filler, side, dtype, n, path, method, packed):
    """1: results() right after run(hip_stream=side), the filler ahead on `side`, through every way a batch answers."""
    from sushi_amd.device import SearchBatch
    want = reference(dtype, "A", n, path, method)
    b = SearchBatch(devs[dtype], devs[dtype], *_requests("A", n), path=path, method=method, **DROP_IN)
    if not packed:
        b.set_packed_output(None)
    assert (b._early is not None) == (n == 3 and path == "fft") and (b._host_rec is not None) == (n == 3)
    assert (b._packed is not None) == (n == 6 and packed)
    _poison(b)
    filler(side)
    b.run(hip_stream=side.cuda_stream)
    assert side.query() is False
    got = b.results()
    print(dtype, n, path, method, packed, got, want)
    assert _same(got, want)
    if dtype == "uint8":
        row = rows[dtype]
        offs, lens, wst, npos = _requests("A", n)
        for k in range(n):
            res = oracle.match_template_direct(row[wst[k]:wst[k] + npos[k] + lens[k] - 1], row[offs[k]:offs[k] + lens[k]], method=method)[0]
            best = int(res.argmin() if method == "sqdiff_normed" else res.argmax())
            assert int(got[0][k]) == best and _bits(got[1])[k] == np.float32(res[best]).view(np.uint32), (k, got, best, res[best])


# (test 2) three more copies of every pattern of A's first three searches inside its own window, each under noise of its own level:
# (position in the stream, standard deviation), clear of one another and of the patterns' own places
NEAR_COPIES = [[(160000, 0.02), (170000, 0.03), (180000, 0.04)], [(195000, 0.02), (200000, 0.03), (205000, 0.04)],
               [(121500, 0.02), (128000, 0.03), (142000, 0.04)]]


@pytest.mark.parametrize("method", METHODS)
def test_threshold_and_best_runs_on_a_side_stream(rows, filler, side, method):
    """2: run_threshold, run() and run_best on `side`, one workspace for all three: the current-stream tensors byte for byte (the
    records a run writes -- the rest of `hits` is unwritten by contract).  Every pattern has three noisy copies in its window
    besides the exact one (they score 0.001 .. 0.006 / 0.98 .. 0.995 where unrelated noise scores 0.25 / 0): the threshold lies
    between, four hits a search; the best three are the exact copy and the two cleaner ones."""
    import torch
    from sushi_amd.device import DeviceStream, SearchBatch
    k, cap = 3, 8
    req = _requests("A", 3)
    row = rows["float32"].copy()
    rng = np.random.default_rng(52)
    for o, m, copies in zip(req[0], req[1], NEAR_COPIES):
        for pos, sd in copies:
            row[pos:pos + m] = (row[o:o + m] + rng.standard_normal(m) * sd).clip(0, 1).astype(np.float32)
    dev = DeviceStream(row)
    thr = 0.05 if method == "sqdiff_normed" else 0.5
    ref = SearchBatch(dev, dev, *req, path="fft", method=method, **DROP_IN)
    ref.run()
    want = tuple(x.copy() for x in ref.results())
    assert list(want[0]) == ANSWER["A"][:3]
    th, tc = ref.run_threshold(thr, cap)
    bh, bc = ref.run_best(k)
    torch.cuda.synchronize()
    th, tc, bh, bc = (x.cpu().numpy() for x in (th, tc, bh, bc))
    print(method, thr, tc, bc, th[:, :, 0], bh[:, :, 0])
    assert (tc == 4).all() and (bc == k).all()
    for j in range(3):
        places = sorted([ANSWER["A"][j]] + [pos - req[2][j] for pos, _ in NEAR_COPIES[j]])
        assert list(th[j, :4, 0]) == places and list(bh[j, :, 0]) == [ANSWER["A"][j]] + [pos - req[2][j] for pos, _ in NEAR_COPIES[j][:2]]
    b = SearchBatch(dev, dev, *req, path="fft", method=method, **DROP_IN)
    _poison(b)
    filler(side)
    gh, gc = b.run_threshold(thr, cap, hip_stream=side.cuda_stream)
    b.run(hip_stream=side.cuda_stream)
    hh, hc = b.run_best(k, hip_stream=side.cuda_stream)
    assert side.query() is False
    side.synchronize()
    gh, gc, hh, hc = (x.cpu().numpy() for x in (gh, gc, hh, hc))
    assert gc.tobytes() == tc.tobytes() and hc.tobytes() == bc.tobytes()
    for j in range(3):
        assert gh[j, :tc[j]].tobytes() == th[j, :tc[j]].tobytes() and hh[j, :bc[j]].tobytes() == bh[j, :bc[j]].tobytes(), j
    assert _same(b.results(), want)


@pytest.fixture(scope="module")
def lanes_job():
    """The 64-event job, the workspace cap under which it takes four sub-batches on two lanes, and a 1:1 batch's bits."""
    from test_pair_exclusion import _audio_like_job
    from sushi_amd.device import SearchBatch
    dst, src, offs, lens, wst, npos, planted = _audio_like_job(n_events=64)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("SUSHI_HIP_LANES", "1:1")
        one = SearchBatch(dst.device_stream(), src.device_stream(), offs, lens, wst, npos, path="fft")
        assert (one.sub_batches, one.lanes) == (1, 1)
        one.run()
        idx, score = one.results()
    assert all(abs(int(i) - p) <= 1 for i, p in zip(idx, planted))
    idx, bits = idx.copy(), _bits(score.copy())
    idx.setflags(write=False); bits.setflags(write=False)
    return (dst.device_stream(), src.device_stream(), offs, lens, wst, npos), int(one.ws_bytes * 0.6), (idx, bits)


def _lanes_batch(monkeypatch, lanes_job, **kw):
    from sushi_amd.device import SearchBatch
    args, cap, ref = lanes_job
    monkeypatch.setenv("SUSHI_HIP_LANES", "4:2")
    b = SearchBatch(*args, path="fft", workspace_bytes=cap, **kw)
    assert b.lanes == 2 and b.sub_batches == 4 and b._packed is not None
    return b, ref


@pytest.mark.parametrize("form", ["band", "whole", "never"])
def test_what_follows_a_lanes_run_on_a_side_stream_follows_all_of_it(monkeypatch, lanes_job, filler, side, form):
    """3: the header's promise for a batch on lanes -- what is ordered behind the run on `hip_stream` is ordered behind all of
    it -- with `hip_stream` a stream of the caller's: clones enqueued on `side` right behind the run hold the 1:1 bits.  Two
    runs of every form: the first whole-row run takes another cut of the plan and uploads it on the run's stream."""
    import torch
    from sushi_amd import _native
    b, ref = _lanes_batch(monkeypatch, lanes_job)
    _native.check(_native.lib().sushi_hip_batch_set_exclusion(b.handle, _native.EXCLUSION[form]), "set_exclusion")
    for r in range(2):
        _poison(b)
        filler(side)
        b.run(hip_stream=side.cuda_stream)
        with torch.cuda.stream(side):
            ci, cs, cp = b.out_idx.clone(), b.out_score.clone(), b._packed.clone()
        assert side.query() is False, (form, r)
        side.synchronize()
        ci, cs, cp = ci.cpu().numpy(), cs.cpu().numpy(), cp.cpu().numpy()
        assert (ci == ref[0]).all() and (_bits(cs) == ref[1]).all(), (form, r)
        assert (cp[:, 0] == ref[0]).all() and (_bits(cp[:, 1]) == ref[1]).all(), (form, r)


# ---- B. a run that was not collected, and a batch re-planned under it ----

def test_every_early_record_that_says_ready_holds_this_runs_answer(devs, reference, filler):
    """4: filler, run() of A, filler, reset(B), run(), all on the current stream, A never collected.  Until the stream has
    drained the host samples the early records through the accessor results() polls (early_ready): whatever counts as ready is
    B's answer -- never A's, whose refine_kernel had not executed when B's run cleared the records.
    The premise -- A still pending -- is asserted BEFORE reset(B) and cannot sit later: the rule under test is that reset() of an
    uncollected batch with early records waits for A, so behind it nothing of A is pending any more and the sampling only
    ever overlaps B.  The test therefore bites on a batch that does not wait: there the samples taken while the second filler runs
    show A's record as ready (profiles/batch_streams/README.md has that failure, recorded on the code before the rule)."""
    import torch
    from sushi_amd.device import SearchBatch
    dev = devs["float32"]
    want = reference("float32", "B", 2)
    assert not _same(reference("float32", "A", 2), want)
    b = SearchBatch(dev, dev, *_requests("A", 2), path="fft", headroom=4.0, **DROP_IN)
    assert b._early is not None
    _poison(b)
    cur = torch.cuda.current_stream()
    filler(cur)
    b.run()
    filler(cur)
    assert cur.query() is False                            # A has not executed: it is behind the first filler still
    assert b.reset(*_requests("B", 2))
    b.run()
    e = b._early.numpy()
    samples, seen, t_end = 0, 0, time.perf_counter() + 5.0
    while True:
        drained = cur.query()
        ready = b.early_ready().copy()                     # (ready first: a record read after its ready word is no older than it)
        rec = e.copy()
        samples += 1
        for k in np.flatnonzero(ready):
            seen += 1
            assert rec[k, 3] == 0 and rec[k, 0] == want[0][k] and rec[k, 1].view(np.uint32) == _bits(want[1])[k], (samples, k, rec, want)
        if drained:
            break
        assert time.perf_counter() < t_end
    print("samples", samples, "ready records seen", seen)
    assert ready.all()
    assert _same(b.results(), want)


@pytest.mark.parametrize("refused", [False, True], ids=["replanned", "refused"])
def test_a_replan_does_not_reach_into_a_pending_run(devs, reference, filler, side, refused):
    """5: A pending on `side` behind the filler, reset from the current stream.  A run that has not executed reads its
    descriptors when it does: re-planned to B under it, it would answer B.  The clones behind it on `side` hold A's answer,
    and the batch then answers B -- or, where the reset is refused (requests too large for the batch), A as before."""
    import torch
    from sushi_amd.device import SearchBatch
    dev = devs["float32"]
    a, bb = reference("float32", "A", 3), reference("float32", "B", 3)
    assert (a[0] != bb[0]).all()
    b = SearchBatch(dev, dev, *_requests("A", 3), path="fft", headroom=1.0 if refused else 4.0, **DROP_IN)
    _poison(b)
    filler(side)
    b.run(hip_stream=side.cuda_stream)
    with torch.cuda.stream(side):
        ci, cs = b.out_idx.clone(), b.out_score.clone()
    assert side.query() is False
    if refused:
        assert b.reset(*TOO_LARGE) is False
    else:
        assert b.reset(*_requests("B", 3)) is True
    b.run()
    got = b.results()
    side.synchronize()
    print(refused, got, ci, cs)
    assert _same(got, a if refused else bb)
    assert _same((ci.cpu().numpy(), cs.cpu().numpy()), a)


@pytest.mark.parametrize("path", ["fft", "direct"])
def test_runs_nobody_collected_change_nothing(devs, reference, path):
    """6: three run() calls back to back, then results(): one run's bits (the drop-in sized batch, either path).  On the FFT
    path this batch has early records, so its second and third run() each wait for the uncollected run before them (the
    class docstring's rule): the three runs follow one another there and are pending together only on the direct path and in
    the lanes test below -- this is no test of overlapping runs on a batch with early records, which the rule does not allow."""
    from sushi_amd.device import SearchBatch
    dev = devs["float32"]
    b = SearchBatch(dev, dev, *_requests("A", 3), path=path, **DROP_IN)
    _poison(b)
    for r in range(3):
        b.run()
    assert _same(b.results(), reference("float32", "A", 3, path))


def test_uncollected_lanes_runs_absorb_each_others_counts_and_change_nothing(monkeypatch, lanes_job):
    """6, the lanes batch in `auto` exclusion: the second and third run take up what the first one's exclusion left (its counts
    come back through pinned words behind an event that is only queried) -- the 1:1 bits all the same."""
    b, ref = _lanes_batch(monkeypatch, lanes_job, exclusion="auto")
    _poison(b)
    for r in range(3):
        b.run()
    idx, score = b.results()
    assert (idx == ref[0]).all() and (_bits(score) == ref[1]).all()
