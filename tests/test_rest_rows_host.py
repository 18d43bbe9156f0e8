"""The survivors' pass of the band-split form on the CPU (sushi_amd/csrc/run_policy.hpp): which unit of work it takes
(rest_rows_route: SUSHI_HIP_REST_ROWS) and the cut of a search's pairs to form into its work items -- runs of at most C pairs to
form, the audit pair left out, nothing for a search with nothing to form -- as the device's builder and consumer walk it
(tests/host_rest_rows_check.cpp, built with g++ and run as a program), against a plain restatement here."""
import os
import subprocess

import numpy as np

from host_checks import PLAIN, SANITIZED

HERE = os.path.dirname(os.path.abspath(__file__))


def _build(out_dir, flags, name):
    exe = os.path.join(str(out_dir), name)
    subprocess.check_call(["g++"] + flags + [os.path.join(HERE, "host_rest_rows_check.cpp"), "-o", exe])
    return exe


def _restated(per_item, audit, marks):
    form = [i for i, m in enumerate(marks) if m and i != audit]
    return [form[j:j + per_item] for j in range(0, len(form), per_item)]


def _marks(n, listed):
    m = [0] * n
    for i in listed:
        m[i] = 1
    return m


def _cases(C):
    """(pairs per item, audit pair, marks) -- 0, 1, C and C + 1 pairs to form; runs that straddle pairs 63 / 64 and 255 / 256 (the
    builder's and the consumer's 64-pair steps); the audit pair first, last, the only listed pair, not listed at all."""
    out = []
    for n in (1, 40, 64, 65, 300):
        for count in (0, 1, C, C + 1, 2 * C + 1):
            if count <= n:
                out.append((C, -1, _marks(n, range(count))))                                  # from the front
                out.append((C, -1, _marks(n, range(n - count, n))))                           # up to the search's end
                out.append((C, -1, _marks(n, [(i * n) // max(count, 1) for i in range(count)])))   # spread out
    for edge in (64, 256):
        for before in range(0, C + 1):                  # the run begins `before` pairs in front of the edge, at every rank of its item
            for lead in range(0, C):
                listed = list(range(lead)) + list(range(edge - before, edge - before + C + 1))
                out.append((C, -1, _marks(300, sorted(set(listed)))))
        out.append((C, -1, _marks(300, [edge - 1, edge])))
        out.append((C, edge - 1, _marks(300, [edge - 1, edge])))
        out.append((C, edge, _marks(300, [edge - 1, edge])))
        out.append((C, -1, _marks(400, [3, edge + 70])))                                       # an item whose pairs lie more than 64 apart
    listed = [2, 5, 6, 7, 30, 31, 39]
    for audit in (2, 39, 6, 0, 38):                     # first, last, inside, not listed (pair 0), not listed (next to the last)
        out.append((C, audit, _marks(40, listed)))
    out.append((C, 17, _marks(40, [17])))               # the only listed pair: nothing to form
    out.append((C, 17, _marks(40, [])))
    out.append((C, 0, _marks(1, [0])))
    out.append((C, -1, []))                              # (a search without pairs does not exist; the walk must not mind)
    out.append((C, -1, _marks(300, range(300))))        # every pair listed: what a dense candidate whose flag is cleared leaves
    out.append((C, 299, _marks(300, range(300))))
    rng = np.random.default_rng(1234 + C)
    for _ in range(40):
        n = int(rng.integers(1, 400))
        marks = (rng.random(n) < rng.choice([0.02, 0.2, 0.6])).astype(int).tolist()
        out.append((C, int(rng.integers(-1, n)), marks))
    return out


def _run_cut(exe, cases, want_clean_stderr):
    text = "".join("%d %d %s\n" % (c, a, "".join(map(str, m)) or "-") for c, a, m in cases)
    r = subprocess.run([exe, "cut"], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and (r.stderr == "" or not want_clean_stderr), r.stdout[-2000:] + r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases)
    return [[[int(p) for p in item.split()] for item in line.split("|")] if line else [] for line in lines]


def test_the_route_rule_passes_its_checks(tmp_path):
    r = subprocess.run([_build(tmp_path, PLAIN, "host_rest_rows_check")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_cut_is_the_restated_cut_and_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The program with its own sanitizer runtime, run stand-alone: the route rule, then every case's items equal to the
    restatement's -- for the three values of C that were measured and for the constant the library is built with."""
    exe = _build(tmp_path, SANITIZED, "host_rest_rows_check_san")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    built_with = int(subprocess.check_output([exe, "pairs"]))
    assert built_with in (2, 4, 8)
    for C in (2, 4, 8):
        cases = _cases(C)
        if C == built_with:
            cases += [(0, a, m) for _, a, m in cases]          # (0: the constant itself)
        got = _run_cut(exe, cases, True)
        for (c, audit, marks), items in zip(cases, got):
            want = _restated(c or built_with, audit, marks)
            assert items == want, (c, audit, "".join(map(str, marks)), items, want)
            assert all(1 <= len(it) <= (c or built_with) for it in items)
            assert (not items) == (not any(m and i != audit for i, m in enumerate(marks)))
