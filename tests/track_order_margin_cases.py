"""What tests/test_track_order_margins_host.py and tests/test_track_order_margins_gpu.py share: the planted scenario in which plain
margins understate what the ordered model gives, the recorded margins of the decoy scenario (tests/track_order_cases.py), and the
tables of the synthetic sequences."""
import numpy as np

import track_margin_cases
import track_order_cases

# ---------------------------------------------------------------------------------------------- two explanations, mirrored
# track_margin_cases' planted scenario with the destination mirrored: 6 rows of 401 shifts, 0.9 everywhere, 0.10 at HERE = 300 and
# 0.12 at THERE = 100; the anchor row's value at THERE is 0.9.  Penalty 0.3, step_cost 0.002, reach 4, guard 20.  Every event is
# placed at 300 and every alternative is 100.  Without a limit the margins are the plain pass's: events 3 .. 5 reach 100 by one jump
# down after the anchor.  With back 50 for every event a jump from 300 down to 100 does not exist, so events 3 .. 5 reach 100 only
# if the whole run goes there, past the anchor: 0.90 each.  Without the anchor every margin is 6 x 0.02 = 0.12 with either back.
PLANT_N, PLANT_E, PLANT_HERE, PLANT_THERE, PLANT_ANCHOR = 401, 6, 300, 100, 2
PLANT_PENALTY, PLANT_STEP_COST, PLANT_REACH, PLANT_GUARD = (track_margin_cases.TWO_PENALTY, track_margin_cases.TWO_STEP_COST,
                                                            track_margin_cases.TWO_REACH, track_margin_cases.TWO_GUARD)
PLANT_BACK = 50
PLANT_MARGINS_PLAIN = [0.32, 0.34, 0.90, 0.36, 0.34, 0.32]         # to six places: back -1, and track_margins_host
PLANT_MARGINS_ORDERED = [0.32, 0.34, 0.90, 0.90, 0.90, 0.90]       # to six places: back 50
PLANT_MARGIN_NO_ANCHOR = 0.12


def planted(anchor=PLANT_ANCHOR):
    """PLANT_E rows of PLANT_N shifts: 0.9 everywhere but 0.10 at PLANT_HERE and 0.12 at PLANT_THERE; row `anchor`'s value at
    PLANT_THERE is 0.9 (None: no anchor)."""
    rows = [np.full(PLANT_N, 0.9, np.float32) for _ in range(PLANT_E)]
    for e, r in enumerate(rows):
        r[PLANT_HERE] = np.float32(0.10)
        if e != anchor:
            r[PLANT_THERE] = np.float32(0.12)
    return rows


# ---------------------------------------------------------------------------------------------- the decoy scenario
# track_order_cases' ten events at its PENALTY (0.02), reach 0, equal weights, step_cost 0, its backs (order_back of the events) and
# GUARD samples: recorded from the oracle's rows by track_ordered_margins_host.  The path is track_order_cases.TRUE_K and every through
# equals the total.  Event 2's alternative is its decoy (-5400), and event 0 goes there with it; event 7's is its decoy (6600).  The
# smallest margins are event 1's (a chance match) and event 8's.
GUARD = 120
COST = track_order_cases.RESULTS[track_order_cases.PENALTY][3]
THROUGH = [3.9198649418354035] * 10
ALT = [4.016639360189438, 3.9462900137901307, 4.016639360189438, 3.9765113270282746, 4.0865828478336335, 4.079671242237091,
       3.993393359184265, 4.029862282276154, 3.9483235156536103, 4.029862282276154]
MARGINS = [0.09677441835403444, 0.02642507195472721, 0.09677441835403444, 0.05664638519287113, 0.16671790599823, 0.15980630040168764,
           0.07352841734886173, 0.1099973404407506, 0.028458573818206823, 0.1099973404407506]
ALT_K = [-5400, 6347, -5400, -475, 3933, -2830, 878, 6600, -4980, 9058]


# ---------------------------------------------------------------------------------------------- synthetic sequences
guards = track_margin_cases.guards


def sequence(E, n, reach, method, seed=0):
    """track_order_cases.sequence with a guard per row: (curves, rows, weights, penalties, reaches, step_cost, backs, guards); the
    penalty of row 0 is 0 (the margins' tables are read from entry 1 on, and a table entry must be a number)."""
    curves, rows, weights, lams, rs, mu, back = track_order_cases.sequence(E, n, reach, method, seed=seed)
    return curves, rows, weights, [0.0] + lams[1:], rs, mu, back, guards(E, n)


def suffix_tie_rows(n, at, method):
    """Three rows of n shifts (weights 1) whose last row holds its minimum, 0.25, twice: at at - 1 and at (255 | 256 and 511 | 512 are
    the two sides of a wave's, a round's or a work item's boundary); everything else in [0.5, 0.75)."""
    rng = np.random.default_rng(n * 11 + at)
    sign = np.float32(-1.0 if method == "ccoeff_normed" else 1.0)
    rows = [rng.random(n, dtype=np.float32) * np.float32(0.25) + np.float32(0.5) for _ in range(3)]
    rows[2][[at - 1, at]] = np.float32(0.25)
    return [r * sign for r in rows]
