"""What tests/test_clamped_rows_host.py and tests/test_clamped_rows_gpu.py share: the synthetic hit lists of the kernel tests, and the
streams, events and clamps of the event_rows and find_* tests."""
import numpy as np

from sushi_amd import rows, synth
from sushi_amd.wav import WavStream

T = rows.TILE
SENTINEL_BITS = 0x7fc00123                          # a NaN no score has: the floats between rows
FILL = np.float32(0.3125)


# ---------------------------------------------------------------------------------------------- synthetic hit lists
def _scores(rng, count, f):
    """Random float32 scores in [-1, 1), among them -0.0, 0.0 and f itself."""
    s = (rng.random(count, dtype=np.float32) * np.float32(2.0) - np.float32(1.0)).astype(np.float32)
    for at, v in zip(range(0, count, 5), (np.float32(-0.0), np.float32(0.0), np.float32(f))):
        s[at] = v
    return s


def _edges(n_pos):
    """Indices on both sides of every tile boundary of a row, and its two ends."""
    at = {0, n_pos - 1}
    for b in range(T, n_pos, T):
        at |= {b - 1, b}
    return sorted(at)


def _call(lists, n_pos, capacity, f, seed):
    """One call: lists[k] is (indices, count) of row k -- count None: len(indices).  Rows lie at odd float offsets in shuffled order,
    one to five sentinel floats between them.  -> dict(hits, counts, table, n_out, f, capacity)."""
    rng = np.random.default_rng(seed)
    n = len(lists)
    hits = np.full((n, capacity, 2), -7, np.int32)          # (records beyond a count are never read: an index no row has)
    counts = np.zeros(n, np.int64)
    offs, at = np.zeros(n, np.int64), 1
    for k in rng.permutation(n):
        offs[k] = at
        at += n_pos[k] + 1 + 2 * int(rng.integers(0, 3))
        at += (at + 1) % 2
    for k, (idx, count) in enumerate(lists):
        idx = np.asarray(idx, np.int64)
        hits[k, :idx.shape[0], 0] = idx
        hits[k, :idx.shape[0], 1] = _scores(rng, idx.shape[0], f).view(np.int32)
        counts[k] = idx.shape[0] if count is None else count
    return dict(hits=hits, counts=counts, table=rows.rows_table(offs, n_pos), n_out=int(at) + 3, f=np.float32(f), capacity=capacity)


SIZES = [1, 2, T - 1, T, T + 1, 3 * T + 5]


def synthetic_calls():
    """The calls of the kernel test: every size of SIZES with an empty list, one hit at index 0, one at n_pos - 1, hits on both
    sides of every tile boundary and every position a hit -- under a capacity of 3 T + 5, which the largest row's full list meets
    exactly (no overflow); a capacity of 4 met exactly and exceeded by one (overflow: the row is all f), with an index at n_pos, a
    negative one, a descending pair and a negative count (bad lists); capacity 0 with and without hits."""
    big, lists, n_pos = 3 * T + 5, [], []
    for n in SIZES:
        for idx in ([], [0], [n - 1], _edges(n), list(range(n))):
            lists.append((idx, None))
            n_pos.append(n)
    calls = [_call(lists, n_pos, big, FILL, seed=1)]
    n = T + 1
    calls.append(_call([([0, T - 1, T], None), ([0, 1, T - 1, T], None), ([0, 1, T - 1, T], 5), ([0, 1, T - 1, T], 10 ** 12),
                        ([3, n], None), ([-1, 3], None), ([0, T, T - 1], None), ([5], -1), ([0, 7, 9], None)],
                       [n] * 9, 4, FILL, seed=2))
    calls.append(_call([([], None), ([], 3), ([], None)], [1, T + 1, 2 * T], 0, np.float32(-0.0), seed=3))
    return calls


def expected(call):
    """(out, flags) of a call by rows_from_hits_host, the output pre-filled with the sentinel."""
    out = np.full(call["n_out"], SENTINEL_BITS, np.uint32).view(np.float32)
    flags = rows.rows_from_hits_host(call["hits"], call["counts"], call["table"], call["f"], out)
    return out, flags


def outside_rows(call):
    """bool[n_out]: the floats no row of the call covers."""
    mask = np.ones(call["n_out"], bool)
    for o, n in zip(call["table"]["out_off"], call["table"]["n_pos"]):
        mask[int(o):int(o) + int(n)] = False
    return mask


# ---------------------------------------------------------------------------------------------- streams
# Seven events of 0.2 - 0.3 s (source times) in streams of 8 s at 12 kHz; the source is the destination advanced by OFFSET samples
# with 20 dB of white noise.  Event TWICE's destination segment is copied a second time TWICE_AT samples off its place (two peaks in
# its +-0.5 s window); event ABSENT's source samples are replaced by other noise (nothing in its window resembles it).
RATE, SECONDS, OFFSET, WINDOW = 12000, 8, 700, 0.5
EVENTS = [(1.0, 1.25), (1.8, 2.1), (2.6, 2.8), (3.4, 3.7), (4.3, 4.55), (5.2, 5.5), (6.1, 6.35)]
TWICE, TWICE_AT, ABSENT = 3, -3100, 4
SEED = 41
# The destination is white noise through an 8-tap mean, so a peak is a few positions wide.  By the CPU oracle's rows, in both sample
# types, the events' hit counts at these clamps are HITS: a lone peak's hits fit CAPACITY, the two peaks of TWICE do not, and ABSENT
# (under 'sqdiff_normed' also the quiet event 2) has none.  tests/test_clamped_rows_host.py checks that against the oracle.
CLAMPS = {"ccoeff_normed": 0.6, "sqdiff_normed": 0.6}
CAPACITY = {"ccoeff_normed": 6, "sqdiff_normed": 10}
HITS = {"ccoeff_normed": [5, 5, 5, 8, 0, 5, 5], "sqdiff_normed": [9, 7, 0, 18, 0, 5, 7]}
PASS_ALL = {"sqdiff_normed": 3.0, "ccoeff_normed": -2.0}      # a clamp nothing fails
K_LO, N_SHIFT = -6000, 12001                        # joint_window of the scenario
PENALTY, REACH, STEP_COST, MAX_RATE = 0.5, 8, 2.0 ** -10, 2e-3


def streams(sample_type):
    """(destination, source) WavStreams of the scenario."""
    dst_pcm = synth.make_dst_pcm(SECONDS, RATE, seed=SEED).copy()
    s, e = EVENTS[TWICE]
    a, b = int(s * RATE) + OFFSET, int(e * RATE) + OFFSET
    dst_pcm[a + TWICE_AT:b + TWICE_AT] = dst_pcm[a:b]
    src_pcm = synth.make_src_pcm(dst_pcm, OFFSET, seed=SEED + 1)
    s, e = EVENTS[ABSENT]
    other = synth.make_dst_pcm(SECONDS, RATE, seed=SEED + 2)
    src_pcm[int(s * RATE) - 600:int(e * RATE) + 600] = other[int(s * RATE) - 600:int(e * RATE) + 600]
    return (WavStream.from_samples(dst_pcm, RATE, sample_type=sample_type), WavStream.from_samples(src_pcm, RATE, sample_type=sample_type))


def scenario(dst, src):
    """(patterns, centres) of the scenario's events."""
    return [src.get_substream(s, e) for s, e in EVENTS], [s for s, _e in EVENTS]
