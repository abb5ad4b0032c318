"""Light Fisher-z targets (dh_fz_light_kernel): a target of at most FW_DH_LIGHT_DEG level-0 neighbours is run from start to end by one
workgroup in front of the device rounds, which then serve what is left of the slot -- or do not run at all.  Whatever the threshold,
the drivers must hand back the same bytes: edges, directed lists, statistics, p-values, reference-order test counts and job counts,
equal to the threshold-0 run (the rounds alone) and to the oracle.

Which path ran is read off the launch counter: the pre-pass counts one subsets_launches per (chain, round) slot it runs in, the rounds
one per non-empty segment launch -- with every target eligible, subsets_launches IS the number of slots.
"""
from math import comb

import numpy as np
import pytest

import flashweave_jl_amd as fw
from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("pc_off", "pc_idx", "pc_weight", "pc_pval")
DEFAULT = 32  # the compiled-in FW_DH_LIGHT_DEG
ALL = 256     # the clamp, FW_TAB_A / 2: every target of the inputs below


@pytest.fixture(scope="module")
def small():
    counts = synth.generate(400, 300, 11, mode="S")
    data, _, _ = pre.normalize(counts, "fz", prec=32)
    data = np.asfortranarray(data)
    n, p = data.shape
    eng = fw.Engine("fz", n, p, max_k=3)
    eng.set_data(data)
    cm = eng.cor()
    deg = np.diff(eng.pw_univar_neighbors()["off"])
    eng.close()
    return dict(n=n, p=p, cm=cm, deg=deg, orc=O.Oracle("fz", cor_mat=cm, n_obs=n), cache={})


def _run(make_engine, monkeypatch, light_deg, sched="1", **lgl):
    """Two lgl calls on one engine under FW_DH_LIGHT_DEG=light_deg (None: the default) and FW_FZ_SCHED=sched, which must agree to the
    byte: (network, counters of the second call)."""
    if light_deg is None:
        monkeypatch.delenv("FW_DH_LIGHT_DEG", raising=False)
    else:
        monkeypatch.setenv("FW_DH_LIGHT_DEG", str(light_deg))
    monkeypatch.setenv("FW_FZ_SCHED", sched)
    eng = make_engine()
    first = eng.lgl(**lgl)
    eng.reset_counters()
    net = eng.lgl(**lgl)
    cn = eng.counters()
    eng.close()
    assert first["edges"] == net["edges"]
    for key in KEYS:
        assert first[key].tobytes() == net[key].tobytes(), key
    return net, cn


def _same(a, b):
    (na, ca), (nb, cb) = a, b
    assert na["edges"] == nb["edges"]
    for key in KEYS:
        assert na[key].tobytes() == nb[key].tobytes(), key
    assert ca["cond_tests_ref"] == cb["cond_tests_ref"] and ca["subsets_calls"] == cb["subsets_calls"]


def _check_oracle(exp, net, cn):
    assert set(net["edges"]) == set(exp["edges"])
    for e, w in exp["edges"].items():
        assert net["edges"][e] == w
    assert cn["cond_tests_ref"] == exp["n_cond_tests"]


def _from_cm(small, max_k=3, **kw):
    def make():
        eng = fw.Engine("fz", small["n"], small["p"], max_k=max_k, **kw)
        eng.set_cor_mat(small["cm"])
        return eng
    return make


def _reference(small, monkeypatch, ff, R):
    """The threshold-0 run of a schedule (the rounds alone), once per module."""
    key = (ff, R)
    if key not in small["cache"]:
        small["cache"][key] = _run(_from_cm(small), monkeypatch, 0, feed_forward=ff, round_size=R)
    return small["cache"][key]


# (True, 100): four rounds of two chains of 50; (True, 80): five rounds on one chain; (False, 0): one round, two chains of 200
@pytest.mark.parametrize("ff,R,slots", [(True, 100, 8), (True, 80, 5), (False, 0, 2)])
def test_threshold_leaves_the_network_alone(small, ff, R, slots, monkeypatch):
    off = _reference(small, monkeypatch, ff, R)
    dflt = _run(_from_cm(small), monkeypatch, None, feed_forward=ff, round_size=R)
    assert small["deg"].max() <= ALL  # precondition: with 256 every target of this input is eligible
    every = _run(_from_cm(small), monkeypatch, ALL, feed_forward=ff, round_size=R)
    _same(dflt, off)
    _same(every, off)
    exp = small["orc"].learn(max_k=3, feed_forward=ff, round_size=max(R, 1) if ff else 1)
    for net, cn in (off, dflt, every):
        _check_oracle(exp, net, cn)
    # the pre-pass ran in every slot and the rounds in none; switched off, the rounds ran
    assert every[1]["subsets_launches"] == slots
    assert off[1]["subsets_launches"] > slots
    if (small["deg"] <= DEFAULT).any() and (small["deg"] > DEFAULT).any():
        assert slots < dflt[1]["subsets_launches"]


@pytest.mark.parametrize("sched", ["1", "0"])
def test_split_slot(small, sched, monkeypatch):
    # the median degree as the threshold: eligible and other targets share the slots, the rounds run on what the pre-pass left
    med = int(np.median(small["deg"]))
    assert 0 < med <= ALL and (small["deg"] <= med).any() and (small["deg"] > med).any()
    got = _run(_from_cm(small), monkeypatch, med, sched=sched, feed_forward=True, round_size=100)
    _same(got, _reference(small, monkeypatch, True, 100))
    assert got[1]["subsets_launches"] > 8


@pytest.mark.parametrize("max_k", [1, 2, 3])
def test_max_k(small, max_k, monkeypatch):
    net, cn = _run(_from_cm(small, max_k), monkeypatch, ALL, feed_forward=True, round_size=100)
    assert cn["subsets_launches"] == 8
    _check_oracle(small["orc"].learn(max_k=max_k, feed_forward=True, round_size=100), net, cn)


def test_max_tests_inside_a_light_job(small, monkeypatch):
    # 5: nearly every job ends on the cap; and a cap between C(a, 3) and the whole enumeration of a typical list of a variables
    sizes = np.diff(_reference(small, monkeypatch, True, 100)[0]["pc_off"])
    a = max(int(np.median(sizes[sizes > 0])), 4)
    mid = (comb(a, 3) + comb(a, 3) + comb(a, 2) + a) // 2
    assert comb(a, 3) < mid < comb(a, 3) + comb(a, 2) + a
    for mt in (5, mid):
        off = _run(_from_cm(small, max_tests=mt), monkeypatch, 0, feed_forward=True, round_size=100)
        got = _run(_from_cm(small, max_tests=mt), monkeypatch, ALL, feed_forward=True, round_size=100)
        _same(got, off)
        assert got[1]["subsets_launches"] == 8
        _check_oracle(small["orc"].learn(max_k=3, max_tests=mt, feed_forward=True, round_size=100), got[0], got[1])


@pytest.mark.parametrize("no_red_tests", [True, False])
def test_exact_elimination_is_served(small, no_red_tests, monkeypatch):
    # fast_elim = False (and no_red_tests = False with it): the pre-pass takes dh_commit's and dh_advance's exact forms as the rounds
    # do -- served, not gated off, as the launch counter shows.  (The oracle's learn has no such option: the rounds are the reference.)
    lgl = dict(feed_forward=True, round_size=100, fast_elim=False, no_red_tests=no_red_tests)
    off = _run(_from_cm(small), monkeypatch, 0, **lgl)
    got = _run(_from_cm(small), monkeypatch, ALL, **lgl)
    _same(got, off)
    assert got[1]["subsets_launches"] == 8 < off[1]["subsets_launches"]


def test_whitelist_duplicates(monkeypatch):
    # one shared factor: every PC set holds nearly every variable, so from the second round on nearly every candidate is whitelisted and
    # the elimination pools carry second entries (hiton.jl:24-26) up to twice the degree.  max_tests caps the enumerations (C(119, 3)
    # subsets per job otherwise: minutes of oracle); rounds of 40 need the device path's threshold lowered
    rng = np.random.default_rng(7)
    n, p = 2000, 120
    data = (rng.standard_normal((n, 1)) + 0.9 * rng.standard_normal((n, p))).astype(np.float32)
    monkeypatch.setenv("FW_DEV_MIN_TARGETS", "32")
    cms = []

    def make():
        eng = fw.Engine("fz", n, p, max_k=3, max_tests=300)
        eng.set_data(data)
        cms.append(eng.cor())
        return eng

    lgl = dict(feed_forward=True, round_size=40)
    off = _run(make, monkeypatch, 0, **lgl)
    got = _run(make, monkeypatch, ALL, **lgl)
    _same(got, off)
    assert np.diff(got[0]["pc_off"]).max() > p // 2
    assert got[1]["subsets_launches"] == 3 < off[1]["subsets_launches"]  # three rounds on one chain
    exp = O.Oracle("fz", cor_mat=cms[0], n_obs=n).learn(max_k=3, max_tests=300, feed_forward=True, round_size=40)
    _check_oracle(exp, got[0], got[1])


def _degenerate_matrix():
    """24 variables: a constant column, two identical columns, a block on one factor, independent columns; one row and column of the
    matrix NaN on top."""
    rng = np.random.default_rng(3)
    n, p = 300, 24
    data = rng.standard_normal((n, p))
    data[:, 4:12] += 1.2 * rng.standard_normal((n, 1))
    data[:, 0] = 1.0
    data[:, 2] = data[:, 1]
    return n, p, np.asfortranarray(data.astype(np.float32))


@pytest.mark.parametrize("alpha", [0.01, 0.9999])
def test_degenerate_columns(alpha, monkeypatch):
    # NaN-preserving forms and exact ties of the maximum p (the duplicate columns); alpha = 0.9999: nothing stops, every enumeration runs
    # to its end; alpha = 0.01: targets of degree 0 and 1 next to the block's
    n, p, data = _degenerate_matrix()
    monkeypatch.setenv("FW_DEV_MIN_TARGETS", "1")
    eng = fw.Engine("fz", n, p, max_k=3)
    eng.set_data(data)
    cm = eng.cor()
    eng.close()
    cm[13, :] = np.nan
    cm[:, 13] = np.nan

    def make():
        e = fw.Engine("fz", n, p, max_k=3, alpha=alpha)
        e.set_cor_mat(cm)
        return e

    probe = make()
    deg = np.diff(probe.pw_univar_neighbors()["off"])
    probe.close()
    if alpha == 0.01:
        assert (deg == 0).any() and (deg == 1).any()  # precondition of this input
    lgl = dict(feed_forward=True, round_size=12)
    off = _run(make, monkeypatch, 0, **lgl)
    got = _run(make, monkeypatch, ALL, **lgl)
    _same(got, off)
    assert got[1]["subsets_launches"] <= 2 <= off[1]["subsets_launches"]  # two rounds on one chain (none where no target has a candidate)
    exp = O.Oracle("fz", cor_mat=cm, n_obs=n).learn(max_k=3, alpha=alpha, feed_forward=True, round_size=12)
    _check_oracle(exp, got[0], got[1])
