"""What tests/test_track_order_wide_host.py and tests/test_track_order_wide_gpu.py share: synthetic sequences of the wide ordered
pass (track_wide_cases' rows with track_order_cases' backs and penalties), and the scenario that needs both extensions at once with
its recorded oracle results."""
import numpy as np

import track_order_cases as ocases
import track_wide_cases as wcases

LAM = 0.0625                                        # the synthetic sequences' penalty: per row 1, 1/4, 0, 2 and 1/2 times it
MIXED_REACH = wcases.MIXED_REACH
SHAPES = wcases.SHAPES


def guards(E, n):
    """One guard per row: 0, 1, 300 and n by turns."""
    return [(0, 1, 300, n)[e % 4] for e in range(E)]


def sequence(E, n, reach, method, seed=0, kinds=None, at=None):
    """(curves, rows, weights, penalties, reaches, backs, guards): track_wide_cases.sequence -- rows with planted ties, dyadic weights
    -- with track_order_cases' backs (0, 1, 255, 256, n - 1, n + 7 and no limit by turns) and penalties per row; reach: one for
    every row, or one per row."""
    curves, rows, weights = wcases.sequence(E, n, method, seed=seed, kinds=kinds, at=at)
    rs = [0] + ([int(reach)] * (E - 1) if np.ndim(reach) == 0 else [int(r) for r in reach][1:])
    lams = [0.0] + ocases.penalties(E, LAM)[1:]
    return curves, rows, weights, lams, rs, ocases.backs(E, n), guards(E, n)


rows_of = wcases.rows_of

# ---------------------------------------------------------------------------------------------- the scenario
# track_wide_cases' long-gap streams -- ten events in uint8 streams of 36 s at 12 kHz, 21.3 s without an event in front of event 5,
# a shift that wanders and drifts by 1890 samples across that stretch; max_rate 9e-3 gives reach_5 = 2399 -- without event 5's own
# decoy, and with track_order_cases' kind of decoy on one event before the gap and one after it: the destination segments of the
# events VICTIMS are copied DECOYS samples off their true places, inside the +-1 s window, and white noise of standard deviation
# NOISE (int16 units) is added at the true places.  Event 2's decoy lies 9000 samples BELOW its place and the gap in front of event
# 2 is 7200 samples (back_2): the jump into the decoy lowers the shift by more than any cut can.  Event 8's lies 9000 samples ABOVE
# and the gap in front of event 9 is 4800 (back_9): the jump back out of it is the forbidden one.  A path through either decoy needs
# a jump that order_back forbids.  Equal weights, step_cost 0.  The results below are the oracle's (oracle.match_template rows).
RATE, WINDOW = wcases.GAP_RATE, wcases.GAP_WINDOW
EVENTS, TRUE_K = wcases.GAP_EVENTS, wcases.GAP_TRUE_K
K_LO, N_SHIFT = wcases.GAP_K_LO, wcases.GAP_N_SHIFT
MAX_RATE, SLACK = wcases.GAP_MAX_RATE, wcases.GAP_SLACK
REACH, CLIPPED = wcases.GAP_REACH, wcases.GAP_CLIPPED
VICTIMS, DECOYS = (2, 8), (-9000, 9000)
NOISE, SEED = 5000.0, wcases.GAP_SEED + 3
BACK = [None, 4800, 7200, 7199, 6000, 255600, 12000, 6000, 8400, 4800]      # order_back of the events: the gaps (None: no limit)
DECOYED_K = [3000, 3040, -5925, 3050, 2990, 1100, 1055, 1090, 10150, 1200]   # every event's lone arg-min, and the plain wide pass's path
DECOYED_JUMPS = [2, 3, 8, 9]
# (a) at these penalties find_track(wide=True) follows both decoys (four jumps) and the wide ordered pass returns the ten true
# shifts without a jump -- event 5 is entered by a move of 1890 samples; (b) the ordered pass with its reaches clipped to 1024
# returns them too but enters event 5 by a jump: its cost is the wide ordered pass's plus the penalty; (c) find_ordered_track with
# the unclipped reach refuses, naming event 5.
# {penalty: (the plain wide pass's cost, the wide ordered pass's cost)}
PENALTIES = (0.1, 0.15, 0.2)
RESULTS = {0.1: (0.9133666871115564, 1.473374605178833),
           0.15: (1.1133666871115566, 1.473374605178833),
           0.2: (1.3133666871115566, 1.473374605178833)}
PENALTY = 0.2                                       # the one the end-to-end tests use
# Outside that range: at 0.25 the plain wide pass gives up event 2's decoy, and from 0.5 on both passes return the true shifts; at
# 0.05 and below the wide ordered pass goes wrong as well -- it reaches event 2's decoy by two legal descents, misplacing event 1
# at -891 on the way (3000 -> -891 -> -5925: 3891 <= back_1 and 5034 <= back_2), which costs less than the noise at event 2's true
# place (0.455 of score) while penalties are that small.  No reach changes that, and the host test asserts it at 0.05.
PENALTY_TOO_SMALL, DETOUR_K = 0.05, [3000, -891, -5925, 3050, 2990, 1100, 1055, 1090, 1150, 1200]
# (d) margins, guard 120 samples, at PENALTY: under the wide ordered pass the decoyed events' margins are 0.3341 and 0.2151 -- event
# 2's best alternative is a shift of its own run (2949: 126 samples from its place), not its decoy, and event 8's is the decoy
# entered by a jump with event 9 dragged along (10124), the cheapest legal way -- where find_track(wide=True, margins=True), whose
# own path lies ON the decoys, says 0.055 and 0.105: the price of going back to the truth.  At 0.1 and 0.15 (d) does not hold for
# both events: the two-descent detour above is then the cheapest alternative of events 1 and 2 (margins 0.0368 and 0.1868, below
# or near the plain pass's 0.255 and 0.155), so (d) is asserted at PENALTY alone and the detour's margins are asserted as they are.
GUARD = 120
ORDERED_MARGINS = {2: 0.3341, 8: 0.2151}            # +- 0.0005
PLAIN_MARGINS = {2: 0.055, 8: 0.105}
ORDERED_ALT_K = {2: 2949, 8: 10150}
DETOUR_MARGINS = {0.1: 0.0368, 0.15: 0.1868}        # events 1 and 2, at the penalties below PENALTY


def streams(sample_type='uint8'):
    """(destination, source) WavStreams of the scenario."""
    from sushi_amd import synth
    from sushi_amd.wav import WavStream
    dst_pcm = synth.make_dst_pcm(wcases.GAP_SECONDS, RATE, seed=wcases.GAP_SEED).copy()
    cuts = [0] + [int(round((EVENTS[i][1] + EVENTS[i + 1][0]) / 2.0 * RATE)) for i in range(len(EVENTS) - 1)]
    src_pcm = synth.make_src_pcm(dst_pcm, list(zip(cuts, TRUE_K)), seed=wcases.GAP_SEED + 1)
    rng = np.random.default_rng(SEED)
    for victim, decoy in zip(VICTIMS, DECOYS):
        s, e = EVENTS[victim]
        a, b = int(s * RATE) + TRUE_K[victim], int(e * RATE) + TRUE_K[victim]
        dst_pcm[a + decoy:b + decoy] = dst_pcm[a:b]
        noisy = dst_pcm[a:b].astype(np.float64) + rng.standard_normal(b - a) * NOISE
        dst_pcm[a:b] = np.clip(np.round(noisy), -32768, 32767).astype(np.int16)
    return tuple(WavStream.from_samples(pcm, RATE, sample_type=sample_type) for pcm in (dst_pcm, src_pcm))


scenario = wcases.gap_scenario
