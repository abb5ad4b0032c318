"""The tables of tests/fzs_edges_tables.py on the CPU oracle alone: no comparison of tests/test_gpu_fzs_edges.py is vacuous, and the
oracle's `pcor` path (Oracle("fz").set_fz_data: sequential, fully centred Float64 sums, the recursion of StatsBase.partialcor) is pinned
by a numpy.longdouble reference that shares neither its code nor its summation order.

Figures below are the oracle's, measured with these generators (n_obs_min = 20).

Worst absolute deviation of the oracle's statistic from `pcor_ld`, k = 1 .. 5 (the conditional tests of `single_tests` and
`offset_tests`): centred tables 3.1e-15 over the 18 sample counts of N_ALL (at n = 2051); offset tables, n = 255 / 2000:
  ratio 30: 2.2e-15 / 4.9e-15     ratio 1 000: 2.0e-15 / 2.3e-15     ratio 30 000: 6.4e-15 / 1.4e-14
Asserted: 1e-12 on every family.

`nine_jobs` (24 columns, lists of 9): at every n of N_ALL and max_k = 3 / 5 four jobs stop (after 1, 3, 7, 1 tests; at n = 2049 the
third runs on) and four enumerate all 129 / 381 subsets.  Networks of `centred(n, 40)`, edges / level-0 pairs / conditional tests,
feed_forward off | on with rounds of 8:
  n = 255   39 / 116 / 283 | 38 / 116 / 256        n = 2048  39 / 190 / 447 | 37 / 190 / 398
  n = 256   37 / 125 / 285 | 37 / 125 / 257        n = 2049  41 / 184 / 458 | 39 / 184 / 405

Degenerate columns (oracle-defined): see test_degenerate_cases_are_stable."""
import numpy as np
import pytest

from tests import fzs_edges_tables as TB

NMIN = TB.N_OBS_MIN


def _worst(orc, data, tests):
    worst, cnt = 0.0, 0
    for x, y, z in zip(*tests):
        if len(z) == 0:
            continue
        s, r = orc.pcor(x, y, z), TB.pcor_ld(data, x, y, z)
        assert np.isfinite(s) and np.isfinite(r)
        worst = max(worst, abs(s - r))
        cnt += 1
    return worst, cnt


def test_generators_are_what_they_say():
    assert np.finfo(np.longdouble).eps < 1e-18  # 64-bit significand or better: the reference is more precise than what it checks
    for n in TB.N_ALL:
        d = TB.centred(n, TB.P_SINGLE)
        assert d.dtype == np.float32 and d.shape == (n, TB.P_SINGLE) and d.flags.f_contiguous
        r = np.corrcoef(d.astype(np.float64).T)
        np.fill_diagonal(r, 0.0)
        assert 0.5 < np.abs(r).max() < 0.9, (n, np.abs(r).max())
    for n in TB.N_OFFSET:
        c = TB.centred(n, TB.P_SINGLE).astype(np.float64)
        for ratio in TB.RATIOS:
            o = TB.offset(n, TB.P_SINGLE, 0, ratio)
            assert o.dtype == np.float32
            o = o.astype(np.float64)
            got = o.mean(axis=0) / o.std(axis=0)
            assert np.all(np.abs(got / ratio - 1.0) < 0.2), (n, ratio, got)
            # the same columns, moved: the Float32 cast of the moved column keeps 2^-9 at worst
            assert np.abs((o - o.mean(axis=0)) - (c - c.mean(axis=0))).max() < 4e-3
    for n in TB.N_LISTS:
        g = TB.degenerate(n)
        assert (g[:, TB.CONST_COL] == np.float32(TB.CONST_VALUE)).all()
        assert g[:, TB.TWIN_COL].tobytes() == g[:, TB.TWIN_SRC].tobytes() and TB.TWIN_COL != TB.TWIN_SRC
    X, Y, Zs = TB.single_tests()
    assert {len(z) for z in Zs} == {0, 1, 2, 3, 4, 5} and (len(X) - 1) % 4 != 0 and len(X) % 4 != 0
    X3, Y3, Zs3 = TB.single_tests(kmax=3, count=31, seed=2)
    assert {len(z) for z in Zs3} == {0, 1, 2, 3} and (len(X3) - 1) % 4 != 0 and len(X3) % 4 != 0
    assert {len(z) for z in TB.offset_tests()[2]} == {1, 2, 3}
    ms = {a + 2 for a in TB.LIST_LENGTHS}
    assert {79, 80, 81, 82} <= ms and {4, 8, 12, 16, 80} <= ms and {3, 5} <= ms  # both sides of the LDS limit; multiples of 4 and not


@pytest.mark.parametrize("n", TB.N_ALL)
def test_oracle_against_longdouble_on_centred_tables(n):
    """k = 1 .. 5 at every n of the GPU module.  Bound 1e-12: the one of the unrounded fz_nz path (tests/test_fznz_edges_cpu.py), a
    tenth of what the device is allowed."""
    orc = TB.oracle_of("centred", n, TB.P_SINGLE)
    data = TB.centred(n, TB.P_SINGLE)
    worst, cnt = _worst(orc, data, TB.single_tests())
    w3, c3 = _worst(orc, data, TB.single_tests(kmax=3, count=31, seed=2))
    print("n = %d: worst deviation %.2e over %d conditional tests" % (n, max(worst, w3), cnt + c3))
    assert cnt >= 30 and max(worst, w3) <= 1e-12
    if n in TB.N_LISTS:  # the degenerate table where the statistic is defined
        g = TB.degenerate(n)
        og = TB.oracle_of("degenerate", n, TB.P_SINGLE, cor="eye")
        for name, x, y, z, kind in TB.DEGENERATE_TESTS:
            if kind == "value":
                assert abs(og.pcor(x, y, z) - TB.pcor_ld(g, x, y, z)) <= 1e-12, name


@pytest.mark.parametrize("n", TB.N_OFFSET)
@pytest.mark.parametrize("ratio", TB.RATIOS)
def test_oracle_against_longdouble_on_offset_tables(ratio, n):
    """Worst deviation of the oracle's conditioned statistic (k = 1 .. 5), n = 255 / 2000:
    ratio 30: 2.2e-15 / 4.9e-15; ratio 1 000: 2.0e-15 / 2.3e-15; ratio 30 000: 6.4e-15 / 1.4e-14.  The oracle centres both factors,
    so the offset costs it nothing but the bits the Float64 difference x - mean loses; asserted 1e-12 as on the centred tables."""
    orc = TB.oracle_of("offset", n, TB.P_SINGLE, ratio, cor="eye")
    data = TB.offset(n, TB.P_SINGLE, 0, ratio)
    w1, c1 = _worst(orc, data, TB.offset_tests())
    w2, c2 = _worst(orc, data, TB.single_tests())
    print("ratio %d, n = %d: worst deviation %.2e over %d conditional tests" % (ratio, n, max(w1, w2), c1 + c2))
    assert c1 == 27 and max(w1, w2) <= 1e-12


def _nine(kind, n, ratio, max_k):
    orc = TB.oracle_of(kind, n, TB.P_SINGLE, ratio, cor="eye")
    T, C, A = TB.nine_jobs()
    return [orc.test_subsets(t, c, a, max_k=max_k, alpha=0.01, n_obs_min=NMIN) for t, c, a in zip(T, C, A)]


@pytest.mark.parametrize("max_k", [3, 5])
@pytest.mark.parametrize("n", TB.N_ALL)
def test_nine_jobs_stop_and_enumerate(n, max_k):
    """Lists of 9: some jobs stop (at rank 0, at rank 2 and at rank 6 of the first run: inside a group of four), some run through all
    129 (max_k = 3) or 381 (max_k = 5) subsets of three or five sizes -- more than 65 ranks, i.e. more than one FZS_RUN of 16 per
    wavefront and more than one sweep of the four wavefronts."""
    res = _nine("centred", n, 0, max_k)
    full = TB.full_count(9, max_k)
    assert full == (129 if max_k == 3 else 381) and full >= 65 and full % 4 != 0  # the enumeration ends inside a group
    stops = [e["num_tests"] for e in res if e["status"] == 1]
    ends = [e for e in res if e["status"] == 2]
    print(n, max_k, stops, len(ends))
    assert len(stops) >= 3 and len(ends) >= 4 and all(e["num_tests"] == full for e in ends)
    assert all(len(e["Zs"]) >= 1 for e in res)
    if max_k == 3:
        assert 1 in stops and 3 in stops and (7 in stops or n == 2049)


@pytest.mark.parametrize("n", TB.N_OFFSET)
@pytest.mark.parametrize("ratio", TB.RATIOS)
def test_nine_jobs_on_offset_tables(ratio, n):
    res = _nine("offset", n, ratio, 3)
    assert sum(e["status"] == 1 for e in res) >= 3 and sum(e["status"] == 2 and e["num_tests"] == 129 for e in res) >= 4


@pytest.mark.parametrize("n", TB.N_LISTS)
def test_list_jobs_cross_the_list_size_switches(n):
    """alpha near 1: the cap ends the long jobs, the short ones enumerate everything; the cap falls inside a group of four for each
    of CAPS_IN_GROUP that is no multiple of 4, and enumerations of 1, 3, 7, 41, 175, 469 subsets end inside one."""
    orc = TB.oracle_of("centred", n, TB.P_LISTS, cor="eye")
    T, C, A = TB.list_jobs()
    assert sorted({len(a) for a in A}) == sorted(TB.LIST_LENGTHS) and len(T) == 2 * len(TB.LIST_LENGTHS)
    capped, whole = 0, 0
    for t, c, a in zip(T, C, A):
        assert len(set(a)) == len(a) and t not in a and c not in a and t != c
        e = orc.test_subsets(t, c, a, max_k=3, alpha=TB.LIST_ALPHA, n_obs_min=NMIN, max_tests=TB.LIST_CAP)
        full = TB.full_count(len(a))
        if len(a) >= 77:
            assert full > TB.LIST_CAP and e["status"] == 1 and e["num_tests"] <= TB.LIST_CAP
            capped += e["num_tests"] == TB.LIST_CAP
        else:
            whole += e["status"] == 2 and e["num_tests"] == full
            assert full % 4 != 0 or len(a) == 0
    assert capped >= 6 and whole >= 9, (capped, whole)
    assert [(c - 1) % 4 for c in TB.CAPS_IN_GROUP] == [0, 1, 2] and TB.LIST_CAP in TB.CAPS_IN_GROUP
    t, c, a = T[-2], C[-2], A[-2]
    for cap in TB.CAPS_IN_GROUP:
        e = orc.test_subsets(t, c, a, max_k=3, alpha=TB.LIST_ALPHA, n_obs_min=NMIN, max_tests=cap)
        assert e["status"] == 1 and e["num_tests"] == cap and len(a) == 80


@pytest.mark.parametrize("n", TB.N_NET)
def test_networks_keep_and_remove_edges(n):
    orc = TB.oracle_of("centred", n, TB.P_NET)
    pairs = len(orc.level0(alpha=0.01, n_obs_min=NMIN)["idx"]) // 2
    for ff, rs in ((False, 0), (True, 8)):
        net = orc.learn(max_k=3, feed_forward=ff, round_size=rs, n_obs_min=NMIN)
        edges = len(net["edges"])
        print("n = %d, feed_forward %s: %d / %d / %d" % (n, ff, edges, pairs, net["n_cond_tests"]))
        assert edges >= 0.1 * pairs and pairs - edges >= 0.1 * pairs and net["n_cond_tests"] >= 100
        assert int(np.diff(net["pc_off"]).max()) >= 3  # subsets of more than one size


@pytest.mark.parametrize("n", TB.N_LISTS)
def test_degenerate_cases_are_stable(n):
    """ORACLE-DEFINED: what fwo_pcor returns where a column is constant, copied or listed twice.  A constant column
    has a zero sum of squares, 0 / 0 = NaN; identical columns give identical sums, s / sqrt(s s) = 1 exactly, and the next step is
    0 / 0 = NaN.  NaN < alpha is false, so a job stops at its first such test, with power.  The twin of a column that is neither X nor
    Y is an ordinary variable: the value of the test on the original."""
    orc = TB.oracle_of("degenerate", n, TB.P_SINGLE, cor="eye")
    for name, x, y, z, kind in TB.DEGENERATE_TESTS:
        s, pv, df, pw = orc.test(x, y, z, n_obs_min=NMIN)
        assert pw and df == 0, name
        if kind == "0/0":
            assert np.isnan(s) and np.isnan(pv), (name, s, pv)
        else:
            z0 = tuple(TB.TWIN_SRC if v == TB.TWIN_COL else v for v in z)
            assert (s, pv) == orc.test(x, y, z0, n_obs_min=NMIN)[:2] and abs(s) > 0.1, (name, s)
        assert (s, pv, df, pw) == orc.test(x, y, z, n_obs_min=NMIN) or np.isnan(s)
    expect = {"a variable twice in the list": (1, 1, (8, 13, 8)), "a variable twice, first and last": (1, 2, (13, 0, 13)),
              "the constant column in the list": (1, 1, (8, 13, TB.CONST_COL)), "the constant column as candidate": (1, 1, (8, 13, 19)),
              "a column and its twin in the list": (1, 2, (13, TB.TWIN_SRC, TB.TWIN_COL))}
    for name, t, c, a in TB.DEGENERATE_JOBS:
        e = orc.test_subsets(t, c, list(a), max_k=3, alpha=0.01, n_obs_min=NMIN)
        assert e["suff_power"]
        if name in expect:
            assert (e["status"], e["num_tests"], e["Zs"]) == expect[name] and np.isnan(e["stat"]) and np.isnan(e["pval"]), (name, e)
        else:
            assert e["status"] == 2 and e["num_tests"] == 7 and np.isfinite(e["stat"]), (name, e)
