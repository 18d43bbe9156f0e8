"""What tests/test_track_margins_host.py and tests/test_track_margins_gpu.py share: the recorded margins of the wandering-shift
scenario (tests/track_cases.py), the planted two-explanation scenario, and the guards of the synthetic sequences."""
import numpy as np

import track_cases

# ---------------------------------------------------------------------------------------------- the wandering-shift scenario
# track_cases' ten events, its REACH, equal weights, at PENALTY, step_cost 0 and GUARD samples: recorded from the oracle's rows by
# track_margins_host.  The path is track_cases.TRUE_K and every through equals the total.  The alternatives of the two victims (events
# 2 and 7) are their decoys, track_cases.LONE_K[2] and LONE_K[7]; the smallest margin is event 6's.
PENALTY, STEP_COST, GUARD = 0.25, 0.0, 120
COST = track_cases.TRACK_COSTS[(PENALTY, STEP_COST)]
THROUGH = [1.983965739607811] * 10
ALT = [2.441821128129959, 2.409272223711014, 2.4259174540638924, 2.415883645415306, 2.416685029864311, 2.4019502848386765,
       2.248919978737831, 2.4215489476919174, 2.511204272508621, 2.3886502236127853]
MARGINS = [0.45785538852214813, 0.4253064841032028, 0.4419517144560814, 0.4319179058074951, 0.43271929025650024, 0.4179845452308655,
           0.26495423913002014, 0.43758320808410645, 0.5272385329008102, 0.40468448400497437]
ALT_K = [3123, 2919, -4125, 2897, 3117, 2965, -2323, 3590, -2229, -2429]

# ---------------------------------------------------------------------------------------------- two explanations, planted
TWO_N, TWO_E, TWO_A, TWO_B = 401, 6, 100, 300
TWO_PENALTY, TWO_STEP_COST, TWO_REACH, TWO_GUARD = 0.3, 0.002, 4, 20


def two_explanations(anchor=None):
    """TWO_E rows of TWO_N shifts: 0.9 everywhere but 0.10 at TWO_A and 0.12 at TWO_B; row `anchor`'s value at TWO_B is 0.9."""
    rows = [np.full(TWO_N, 0.9, np.float32) for _ in range(TWO_E)]
    for e, r in enumerate(rows):
        r[TWO_A] = np.float32(0.10)
        if e != anchor:
            r[TWO_B] = np.float32(0.12)
    return rows


# ---------------------------------------------------------------------------------------------- synthetic sequences
def guards(E, n):
    """One guard per row that varies by row: 0, 1, 300 and n (no shift lies outside) by turns."""
    return [(0, 1, 300, n)[e % 4] for e in range(E)]


def path_terms(got, rows, weights, penalty, step_cost, method="sqdiff_normed"):
    """S of the bound |through_e - cost| <= 6 E 2^-53 S: the sum of the absolute values of the optimal path's terms -- every event's
    weighted score at its shift, the prices of its moves and its penalties."""
    total = 0.0
    for e, s in enumerate(got.shifts):
        total += abs(float(weights[e]) * float(rows[e][s]))
        if e:
            word = int(got.moves[e, s])
            total += float(penalty) if word == -32768 else float(step_cost) * abs(word)
    return total
