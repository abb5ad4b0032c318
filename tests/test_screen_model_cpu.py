"""The Float32 screen of the size-3 Fisher-z kernel (fw_fz_core.h, fz_seg_body, `#if FW_FZ_SCREEN`) attacked on the CPU through its numpy
restatement (tests/screen_model.py): is the hand-derived error term dl = 4.8e-5 / d1 + 7.4e-5, with the guards d1 > 0.01, g > 0.02,
Pb, Pc > dl, Nlo > 0 and the factor 1.0002, large enough that a test the screen skips never has an exact |stat|^2 at or below the bound
it was screened against?  A too-small constant is silent on the device (a wrong edge weight / conditioning set, no fault), and random
well-conditioned data cannot tell the kernel's dl from one four times smaller -- so the operands here are drawn INTO the guard windows and
pushed onto round5 half-points.

The model chooses inputs and counts coverage; the expected value of anything is the oracle's (test_exact_half_equals_the_oracle).
"""
import json
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import screen_model as M
from tests.util import GOLDEN

f32, f64 = np.float32, np.float64
N_SWEEP = 10_000_000  # random tuples over the four guard windows together
CHUNK = 500_000


@pytest.fixture(scope="module")
def sweep():
    """The random sweep, evaluated once: per window and reciprocal variant the screened count inside the window, the violations and the
    smallest ratio exact |stat|^2 / lower bound; a sample of the tuples for the oracle anchor."""
    rng = np.random.default_rng(20240607)
    res = {w: dict(n=0, inwin={u: 0 for u in M.ULPS}, viol={u: 0 for u in M.ULPS}, rmin=np.inf, bad=[], pub_bad=0) for w in M.WINDOWS}
    sample = []
    per = N_SWEEP // len(M.WINDOWS)
    for w in M.WINDOWS:
        for _ in range(per // CHUNK):
            c = M.draw_tuples(rng, CHUNK, w)
            ex = M.exact(**c)
            for u in M.ULPS:
                sc = M.screen(ex, rcp_ulp=u)
                v = M.violations(ex, sc)
                res[w]["inwin"][u] += int((sc["guards"] & M.in_window(sc, w)).sum())
                res[w]["viol"][u] += int(v.sum())
                res[w]["rmin"] = min(res[w]["rmin"], float(M.ratio(ex, sc).min()))
                if v.any() and len(res[w]["bad"]) < 5:
                    i = int(np.flatnonzero(v)[0])
                    res[w]["bad"].append({k: float(c[k][i]) for k in M.OPERANDS})
            with np.errstate(all="ignore"):
                q = ex["ev"] * ex["ev"] / (ex["xb"] * ex["xc"])
                res[w]["pub_bad"] += int(((q > 0.0) & (q < 1.0) & ~(M.published(ex).astype(f64) >= q)).sum())
            res[w]["n"] += CHUNK
            pick = rng.choice(CHUNK, 500, replace=False)
            sample.append({k: c[k][pick] for k in M.OPERANDS})
    return res, {k: np.concatenate([s[k] for s in sample]) for k in M.OPERANDS}


@pytest.fixture(scope="module")
def directed():
    c, est = M.directed_search()
    return c, est, M.critical_scale(c)


def _oracle_stats(c):
    """Oracle.test(X, Y, (z1, zj, zk)).stat for every tuple: 200 tuples per block-diagonal matrix, five variables [X, Y, z1, zj, zk] each."""
    n = len(c["cXY"])
    out = np.empty(n)
    B = 200
    for lo in range(0, n, B):
        hi = min(n, lo + B)
        cm = np.eye(5 * B, dtype=f32)
        for t in range(lo, hi):
            o = 5 * (t - lo)
            cm[o:o + 5, o:o + 5] = M.tuple_matrix(**{k: c[k][t] for k in M.OPERANDS})
        orc = O.Oracle("fz", cor_mat=cm, n_obs=500)
        for t in range(lo, hi):
            o = 5 * (t - lo)
            out[t] = orc.test(o, o + 1, (o + 2, o + 3, o + 4))[0]
        orc.close()
    return out


def test_exact_half_equals_the_oracle(sweep, directed):
    """The model's exact statistic is the oracle's to the bit on 10 000 tuples of the sweep (every window: clamps, NaN from entries
    at +-1, literal 0 / +-1 level-1 values included) and on the whole final population of the directed search."""
    c = {k: np.concatenate([sweep[1][k], directed[0][k]]) for k in M.OPERANDS}
    assert len(c["cXY"]) >= 10_000
    got = M.exact(**c)["stat"]
    exp = _oracle_stats(c)
    same = (got == exp) | (np.isnan(got) & np.isnan(exp))
    bad = np.flatnonzero(~same)
    assert bad.size == 0, [({k: float(c[k][i]) for k in M.OPERANDS}, got[i], exp[i]) for i in bad[:3]]
    assert np.isfinite(got).sum() > 9000 and (np.abs(got) == 1.0).sum() > 10  # (not vacuous: real values, and the clamps are in it)


def test_random_sweep_no_violation_in_any_guard_window(sweep):
    """>= 1e7 random tuples drawn into the guard windows (d1 in [0.009, 0.02]; g in [0.015, 0.04]; Pb or Pc within 2 dl of dl; Nlo within
    2 dl of 0): with the kernel's constants and each of the three reciprocals no tuple that passes every guard has an exact |stat|^2 at
    or below (lower bound) / 1.0002, and the bound the exact path publishes (x 1.00001) is never below the |stat|^2 it stands for.
    Each window holds >= 1 000 tuples that pass every guard inside it -- otherwise the first assertion would be vacuous."""
    res = sweep[0]
    assert sum(r["n"] for r in res.values()) >= 10_000_000
    for w, r in res.items():
        print("window %-2s: %d tuples, pass every guard inside the window %s, violations %s, smallest exact/LB %.6f" %
              (w, r["n"], [r["inwin"][u] for u in M.ULPS], [r["viol"][u] for u in M.ULPS], r["rmin"]))
    for w, r in res.items():
        assert min(r["inwin"].values()) >= 1000, (w, r["inwin"])
        assert sum(r["viol"].values()) == 0, (w, r["viol"], r["bad"])
        assert r["pub_bad"] == 0, w


def test_directed_search_no_violation(directed):
    """The coordinate descent onto round5 half-points (screen_model.directed_search) ends on tuples that pass every guard, and none of
    them -- with the kernel's constants, any of the three reciprocals -- is a violation."""
    c, est, _ = directed
    ex = M.exact(**c)
    screened = 0
    for u in M.ULPS:
        sc = M.screen(ex, rcp_ulp=u)
        v = M.violations(ex, sc)
        assert not v.any(), {k: float(c[k][np.flatnonzero(v)[0]]) for k in M.OPERANDS}
        screened = max(screened, int(sc["guards"].sum()))
    assert screened >= 1000
    # the search did line errors up: its tuples sit closer to the bound than the starts it came from
    start = M.scale_estimate(M.draw_tuples(np.random.default_rng(7), 1000, "d1"))
    assert np.median(est) > np.median(start)


def test_margin_of_dl(sweep, directed):
    """MEASUREMENT (of the model, not asserted as a value): the largest scale s of dl at which a tuple of the directed search is a
    violation.  Measured: s = 0.184 (random tuples of the near-collinear window alone: 0.160; among tuples whose |stat|^2 lies in the
    normal range of p: 0.154) -- the kernel's dl is about five times what the worst operands found need.  Asserted: s < 1, i.e. the kernel's own constants admit no violation in the model."""
    c, _, crit = directed
    s = float(crit.max())
    rnd = M.draw_tuples(np.random.default_rng(11), 200_000, "d1")
    s_rnd = float(M.critical_scale(rnd, iters=10).max())
    i = int(np.argmax(crit))
    print("margin: largest violating scale of dl, directed search s = %.4f (random tuples of the near-collinear window: %.4f)" % (s, s_rnd))
    print("        worst tuple: %s" % {k: float(c[k][i]) for k in M.OPERANDS})
    assert 0.0 < s < 1.0


def test_tie_fixture_is_what_the_selection_says():
    """tests/golden/screen_tuples.json against the committed rule that made it (screen_model.select_tie_tuples; its oracle half -- the job
    is all-significant with the last tied test as its maximum-p test -- is asserted where the fixture is used, tests/test_gpu_fz_screen.py):
    every tuple is a violation of the model somewhere between dl / 20 and dl, none at full size, and the simulated fast loop skips the
    job's maximum-p test with dl at one twentieth and keeps it at full size."""
    with open(os.path.join(GOLDEN, "screen_tuples.json")) as fh:
        tuples = json.load(fh)["tuples"]
    assert len(tuples) >= 20
    c = {k: np.array([t[k] for t in tuples], f32) for k in M.OPERANDS}
    crit = M.critical_scale(c)
    assert (crit >= 0.065).all() and (crit < 1.0).all(), crit
    for t in tuples[::3]:
        r_mut, skipped_mut = M.tie_job_prediction(t, 0.05)
        r_full, skipped_full = M.tie_job_prediction(t, 1.0)
        assert r_mut == r_full == 379 and skipped_mut and not skipped_full, t
