"""The tables of tests/fznz_edges_tables.py on the CPU oracle alone: no comparison of tests/test_gpu_fznz_edges.py is vacuous, and the
oracle's unrounded Float64 path is pinned by a reference that shares neither its code nor its summation order.

Figures below are the oracle's (n_obs_min = 20 unless stated), measured with these generators.

test_subsets jobs of `stair_jobs` (views of column 0 with every staircase column x |accepted| = 0 1 2 3 6 7 14 15), by outcome --
sentinel (empty list) / too few rows, no test / rejected before the last subset / rejected at the last subset / every test significant:

  n        jobs   n_obs_min = 20          n_obs_min = 0           no matrix, 20 (NaN statistics)   no matrix, 0 (NaN statistics)
  130      120    15 / 42 / 32 / 2 / 29   15 / 0 / 68 / 8 / 29    15 / 42 / 32 / 2 / 29  (0)       15 / 0 / 68 / 8 / 29  (26)
  16 384    63     9 / 18 / 11 / 0 / 25    9 / 0 / 25 / 2 / 27     9 / 18 / 14 / 0 / 22  (4)        9 / 0 / 28 / 2 / 24  (15)
  16 385    63     9 / 18 / 17 / 1 / 18    9 / 0 / 32 / 3 / 19     9 / 18 / 19 / 1 / 16  (2)        9 / 0 / 34 / 3 / 17  (13)

Networks of `chain` (16 variables, max_k = 3, feed_forward = False): edges / level-0 pairs / conditional tests
  n = 63      19 /  63 / 184        n = 127     18 /  74 / 205        n = 16 383   17 /  85 / 241
  n = 64      16 /  57 / 142        n = 128     20 / 101 / 311        n = 16 384   17 /  80 / 256
  n = 65      18 /  71 / 207        n = 129     18 /  84 / 209        n = 16 385   17 /  83 / 244
  n = 129, max_k = 5: 18 / 84 / 209 (no list longer than three variables); `staircase` at n = 130: 34 edges, 773 tests with max_k = 3,
  35 edges, 615 tests with max_k = 5.  `hub` (130 x 110, feed_forward = True, rounds of 8): 160 edges, 6 434 617 conditional tests, the
  hub's directed list holds 73 variables.

Order-free reference (`pcor_longdouble`), worst relative deviation of the oracle's statistic without a matrix over the powered tests
of `stair_tests` (k = 0 .. 3): 2.3e-15 at n = 130 (36 tests), 6.2e-14 at n = 16 384 (24), 3.1e-14 at n = 16 385 (24); the two large
figures come from the view of every row, whose sums the oracle runs sequentially over 16 384 terms.  Asserted: 1e-12."""
import collections

import numpy as np
import pytest

from tests import fznz_edges_tables as TB

NMIN = TB.N_OBS_MIN


@pytest.mark.parametrize("n", sorted(TB.SIZES))
def test_staircase_views_have_exactly_the_listed_rows(n):
    data, sizes = TB.staircase(n), TB.SIZES[n]
    assert data.shape == (n, 1 + len(sizes) + TB.N_COND[n]) and data.shape[1] <= (16 if n > 1000 else 24)
    assert data.dtype == np.float32 and (data[:, 0] != 0).all()
    assert tuple(len(TB.view_rows(data, 0, 1 + j)) for j in range(len(sizes))) == sizes
    assert {0, 3, NMIN - 1, NMIN, 64, 65, 129, n} <= set(sizes)
    if n == TB.N_STAIR:  # the small table holds every view size of the list; the large ones have 16 columns for nine of them
        assert {1, 2, 4, NMIN + 1, 63, 127, 128} <= set(sizes)
    cond = TB.stair_cond(n)
    fill = (data[:, cond] != 0).mean(axis=0)
    assert len(cond) >= 6 and 0.7 < fill.min() and fill.max() < 0.9, fill
    # a zero inside a view is a value: every view of 20 rows or more holds zeros of its first conditioning column, and values too
    X, Y, Zs = TB.stair_tests(n)
    for x, y, z in zip(X, Y, Zs):
        rows = TB.view_rows(data, x, y)
        if len(z) and len(rows) >= NMIN:
            col = data[rows, z[0]]
            assert (col == 0).any() and np.count_nonzero(col) >= 2, (n, y, z)


@pytest.mark.parametrize("nmin", [NMIN, 0])
@pytest.mark.parametrize("n", sorted(TB.SIZES))
def test_suff_power_iff_the_view_has_n_obs_min_rows(n, nmin):
    data = TB.staircase(n)
    X, Y, Zs = TB.stair_tests(n)
    for stream in (False, True):
        orc = TB.oracle_of("staircase", n, stream)
        npow = 0
        for x, y, z in zip(X, Y, Zs):
            s, pv, df, pw = orc.test(x, y, z, n_obs_min=nmin)
            nR = len(TB.view_rows(data, x, y))
            assert pw == (nR >= nmin) and df == 0, (n, nmin, x, y, z, nR, pw)
            if not pw:
                assert (s, pv) == (0.0, 1.0)
            if nR <= 3:
                assert pv == 1.0 or np.isnan(pv), (n, nmin, y, z, s, pv)  # sf <= 0: the Fisher-z scale is 0
            npow += pw
        assert npow == 4 * sum(s >= nmin for s in TB.SIZES[n])


def _outcomes(n, nmin, stream):
    orc = TB.oracle_of("staircase", n, stream)
    T, C, A = TB.stair_jobs(n)
    cnt, nnan = collections.Counter(), 0
    for t, c, a in zip(T, C, A):
        e = orc.test_subsets(t, c, a, max_k=3, alpha=0.01, n_obs_min=nmin)
        full = TB.full_count(len(a))
        assert e["num_tests"] <= full
        if e["status"] == 0:
            assert len(a) == 0
            cnt["sentinel"] += 1
        elif e["num_tests"] == 0:
            assert e["status"] == 1 and not e["suff_power"] and len(TB.view_rows(TB.staircase(n), t, c)) < nmin
            cnt["too few rows"] += 1
        elif e["status"] == 1:
            cnt["rejected early" if e["num_tests"] < full else "rejected last"] += 1
        else:
            assert e["status"] == 2 and e["num_tests"] == full
            cnt["all significant"] += 1
        nnan += bool(e["status"] and np.isnan(e["stat"]))
    return len(T), cnt, nnan


@pytest.mark.parametrize("stream", [False, True], ids=["matrix", "no_matrix"])
@pytest.mark.parametrize("nmin", [NMIN, 0])
@pytest.mark.parametrize("n", sorted(TB.SIZES))
def test_jobs_reject_and_enumerate(n, nmin, stream):
    """Shares of the jobs by outcome: rejections and whole enumerations each make up a tenth of the jobs or more (the share asked of
    the networks below), every list size of ACC_SIZES occurs, and with n_obs_min = 0 no job is turned away for too few rows -- the views of 0 .. 4 rows are really tested."""
    njobs, cnt, nnan = _outcomes(n, nmin, stream)
    print(n, nmin, "no matrix" if stream else "matrix", njobs, dict(cnt), "NaN statistics:", nnan)
    views = len(TB.SIZES[n])
    sizes = {len(a) for a in TB.stair_jobs(n)[2]}
    assert sizes == (set(TB.ACC_SIZES) if n == TB.N_STAIR else set(TB.ACC_SIZES) - {15})  # 16 columns: no list of 15 without a repeat
    assert cnt["sentinel"] == views
    small_views = sum(s < nmin for s in TB.SIZES[n])
    assert cnt["too few rows"] == small_views * (len(sizes) - 1)
    assert cnt["rejected early"] + cnt["rejected last"] >= 0.1 * njobs and cnt["all significant"] >= 0.1 * njobs, cnt
    if stream and nmin == 0:
        assert nnan >= 5  # a column that is constant inside a view stops the enumeration with a NaN p-value
    if not stream:
        assert nnan == 0  # the matrix path writes 0 for such a pair


@pytest.mark.parametrize("n", TB.N_SMALL + TB.N_LARGE)
def test_chain_networks_keep_and_remove_edges(n):
    """At least a tenth of the level-0 pairs stay edges and at least a tenth are removed by conditional tests, at every n."""
    orc = TB.oracle_of("chain", n)
    net = orc.learn(max_k=3, feed_forward=False, n_obs_min=NMIN)
    pairs = len(orc.level0(alpha=0.01, n_obs_min=NMIN)["idx"]) // 2
    edges = len(net["edges"])
    print("n = %d: %d / %d / %d" % (n, edges, pairs, net["n_cond_tests"]))
    assert edges >= 0.1 * pairs and pairs - edges >= 0.1 * pairs and net["n_cond_tests"] >= 100, (edges, pairs, net["n_cond_tests"])
    assert TB.chain(n).shape == (n, 16)
    for p in (15, 17, 33) if n == 65 else ():  # level-0 tile counts: some pair is significant in every tile row
        l0 = TB.oracle_of("chain", n, p=p).level0(alpha=0.01, n_obs_min=NMIN)
        assert len(l0["idx"]) >= 2 * (p - 1), (p, len(l0["idx"]))


def test_chain_max_k_5_and_hub():
    net = TB.oracle_of("chain", 129).learn(max_k=5, feed_forward=False, n_obs_min=NMIN)
    assert len(net["edges"]) >= 10 and net["n_cond_tests"] >= 100
    # the chain's lists hold three variables at most; the staircase table's common factor gives lists that subsets of four and five are drawn from
    st3 = TB.oracle_of("staircase", 130).learn(max_k=3, feed_forward=False, n_obs_min=NMIN)
    st5 = TB.oracle_of("staircase", 130).learn(max_k=5, feed_forward=False, n_obs_min=NMIN)
    assert int(np.diff(net["pc_off"]).max()) <= 3 and st5["n_cond_tests"] != st3["n_cond_tests"] and len(st5["edges"]) >= 10
    hub = TB.oracle_of("hub", 130).learn(max_k=3, feed_forward=True, round_size=8, n_obs_min=NMIN, threads=4)
    longest = int(np.diff(hub["pc_off"]).max())
    print("max_k 5: %d edges, %d tests; hub: %d edges, %d tests, longest directed list %d"
          % (len(net["edges"]), net["n_cond_tests"], len(hub["edges"]), hub["n_cond_tests"], longest))
    assert longest > 62 and int(np.argmax(np.diff(hub["pc_off"]))) == 0  # the hub's list passes FZNZ_DEV_SMALL - 2


def test_wide_jobs_cross_the_list_size_switches():
    (T, C, A), (Ts, Cs, As) = TB.wide_jobs()
    assert {62, 63, 64, 512, 513} <= {len(a) for a in A} and max(len(a) for a in As) <= 14
    assert TB.wide().shape == (130, 520)
    orc = TB.oracle_of("wide", 130)
    for t, c, a in zip(T, C, A):
        assert len(set(a)) == len(a) and t not in a and c not in a
        if len(a) >= 62:  # alpha near 1: the cap ends the job, not the first test
            e = orc.test_subsets(t, c, a, max_k=3, alpha=0.9999, n_obs_min=NMIN, max_tests=3000)
            assert e["status"] == 1 and 100 <= e["num_tests"] <= 3000, e


def test_nan_directed_column_is_constant_inside_its_view():
    data, T, Cn, z, others = TB.nan_directed()
    rows = TB.view_rows(data, T, Cn)
    assert len(rows) >= 2 * NMIN and not data[rows, z].any() and np.count_nonzero(data[:, z]) >= 3
    matrix, stream = TB.oracle_of("nan", 65), TB.oracle_of("nan", 65, True)
    s, pv, df, pw = stream.test(T, Cn, (others[0], z), n_obs_min=NMIN)
    assert pw and np.isnan(s) and np.isnan(pv)
    s, pv, df, pw = matrix.test(T, Cn, (others[0], z), n_obs_min=NMIN)
    s1 = matrix.test(T, Cn, (others[0],), n_obs_min=NMIN)[0]
    assert pw and np.isfinite(s) and np.isfinite(pv) and abs(s - s1) < 2e-5  # a correlation of 0 conditions on nothing (5-digit rounding)


@pytest.mark.parametrize("n", sorted(TB.SIZES))
def test_oracle_without_matrix_against_the_order_free_reference(n):
    """oracle (set_fz_nz_stream: sequential Float64 sums, the recursion of StatsBase.partialcor) against numpy.longdouble with pairwise
    sums, k = 0 .. 3 on every powered view.  Bound 1e-12: 1 / 100 of the 1e-10 the device is allowed on this path (RTOL in
    tests/test_gpu_fznz.py) and 16 x the worst deviation measured (module docstring)."""
    assert np.finfo(np.longdouble).eps < 1e-18  # 64-bit significand or better: the reference is more precise than what it checks
    data = TB.staircase(n)
    orc = TB.oracle_of("staircase", n, True)
    X, Y, Zs = TB.stair_tests(n)
    worst, npow = 0.0, 0
    for x, y, z in zip(X, Y, Zs):
        s, pv, df, pw = orc.test(x, y, z, n_obs_min=NMIN)
        if not pw:
            continue
        r, nR = TB.pcor_longdouble(data, x, y, z)
        assert nR >= NMIN and np.isfinite(s) and np.isfinite(r) and abs(r) > 1e-3, (n, x, y, z, s, r)
        worst = max(worst, abs(s - r) / max(abs(s), abs(r)))
        npow += 1
    print("n = %d: worst relative deviation %.2e over %d powered tests" % (n, worst, npow))
    assert npow == 4 * sum(s >= NMIN for s in TB.SIZES[n]) and npow >= 24
    assert worst <= 1e-12, worst
