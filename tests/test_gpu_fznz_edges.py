"""The HE-S ("fz_nz") kernels on and next to every point where the sample count, the rows of a view or the length of an accepted list
switch the code path, against the CPU oracle, through the C ABI.  DESIGN.md section 4.6 lists the switches with the test below that
crosses each; tests/test_fznz_edges_cpu.py asserts on the oracle alone that no comparison here is vacuous (view sizes, power, shares
of rejections and whole enumerations, network sizes) and pins the oracle's unrounded path to an order-free long-double reference.

Tolerances are the project's (tests/test_gpu_fznz.py): on the matrix path statistics, weights, conditioning sets, status, num_tests,
suff_power, CSR lists and test counts are equal (==) and p-values agree to 1e-12 relative; without a matrix (recursive_pcor = False)
statistics follow `_near` (1e-10 relative or 1e-14 absolute) and p-values 1e-12 absolute, against the oracle and, where a test has
power, against the long-double reference as well.  n_obs_min is passed explicitly, the same value to the engine and to the oracle."""
import functools

import numpy as np
import pytest

import flashweave_jl_amd as fw
from tests import fznz_edges_tables as TB
from tests.util import rel

pytestmark = pytest.mark.gpu
NMIN = TB.N_OBS_MIN
RTOL, PTOL = 1e-10, 1e-12
ROUTES = ("host", "tensor", "csc", "csc_resident")
L0_KEYS = ("off", "idx", "stat", "pval")


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _near(a, b):
    return _same(a, b) or rel(a, b) < RTOL or abs(a - b) < 1e-14


def _pclose(a, b):
    return _same(a, b) or rel(a, b) < PTOL


def _engine(data, route="host", nmin=NMIN, **kw):
    """An engine holding `data` through one of the four upload routes: the host loop of fwi_fznz_upload, a torch GPU tensor
    (fznz_dev_plane_kernel), the CSC triple (fznz_csc_scatter_kernel), the triple kept CSC-resident (fznz_cscres_*_kernel)."""
    n, p = data.shape
    eng = fw.Engine("fz_nz", n, p, n_obs_min=nmin, **kw)
    try:
        if route == "host":
            eng.set_data(data)
        elif route == "tensor":
            import torch
            eng.set_data(torch.from_numpy(np.array(data.T, order="C")).to("cuda:0").t())
        else:
            eng.set_data(TB.to_triple(data), csc_resident=route == "csc_resident")
    except Exception:
        eng.close()
        raise
    return eng


# ---- 1. level 0 ----

def _check_level0(data, exp, routes, what):
    assert len(exp["idx"]) > 0, what
    first = None
    for route in routes:
        eng = _engine(data, route, max_k=0)
        try:
            got = eng.pw_univar_neighbors()
        finally:
            eng.close()
        assert np.array_equal(got["off"], exp["off"]) and np.array_equal(got["idx"], exp["idx"]), what + (route,)
        assert np.array_equal(got["stat"], exp["stat"]), what + (route,)
        assert np.allclose(got["pval"], exp["pval"], rtol=PTOL, atol=0), what + (route,)
        if first is None:
            first = got
        for k in L0_KEYS:  # every route leaves the same plane and the same values: the same bytes out
            assert got[k].tobytes() == first[k].tobytes(), what + (route, k)


@pytest.mark.parametrize("n", TB.N_SMALL + TB.N_LARGE)
def test_level0_at_every_n_through_every_upload_route(n):
    """fznz_level0_kernel with the last plane word partial (63, 65, 127, 129, 16 383, 16 385) and full (64, 128, 16 384); each route
    builds the tail of a column's last word itself.  16 383 goes through the host loop alone."""
    routes = ROUTES if n != 16383 else ROUTES[:1]
    exp = TB.oracle_of("chain", n).level0(alpha=0.01, n_obs_min=NMIN)
    _check_level0(TB.chain(n), exp, routes, ("chain", n))


@pytest.mark.parametrize("p", (15, 16, 17, 33))
def test_level0_pair_tiles(p):
    """16 x 16 pair tiles, those on or below the diagonal skipped: one ragged tile, one full tile, 2 x 2 and 3 x 3 tiles with a ragged
    last row and column."""
    exp = TB.oracle_of("chain", 65, p=p).level0(alpha=0.01, n_obs_min=NMIN)
    _check_level0(TB.chain(65, p), exp, ROUTES, ("chain", 65, p))


# ---- 2. single tests and test_subsets jobs on the staircase ----

@functools.lru_cache(maxsize=None)
def _reference(n):
    """pcor_longdouble of every test of stair_tests(n) -> list of (statistic, rows of the view)"""
    data = TB.staircase(n)
    return [TB.pcor_longdouble(data, x, y, z) for x, y, z in zip(*TB.stair_tests(n))]


# Without a matrix the statistic of a view with fewer than k + 2 rows is 0 / 0 in exact arithmetic: two rows make every correlation
# +-1, and in general the k + 2 centred columns span at most nR - 1 dimensions, so some 1 - r^2 of the recursion is exactly 0 under a
# numerator that is exactly 0.  What comes out is the rounding of that step's operands -- NaN where they round to +-1 exactly (the
# oracle's s / sqrt(ss_a ss_b) mostly does), any value clamped into [-1, 1] where they do not (tot / (sd_a sd_b) on the device), and
# the reference's own quotient is a third form.  No tolerance compares such numbers.  The matrix path is not affected: its Float32
# matrix and the oracle's are the same bits, so the same noise comes out of both.  These cases stay in the batch (they reach the
# kernels only with n_obs_min = 0) and everything that is defined is compared: power, df, and the p-value where the view has at most
# three rows, since the Fisher-z scale is then 0 and p is 1 whatever the statistic.
def _defined(nR, k):
    return nR >= k + 2


def _compare_test(g, e, matrix, what, nR=None, k=0):
    assert g.suff_power == e[3] and g.df == 0, what + (g, e)
    if matrix:
        assert _same(g.stat, e[0]) and _pclose(g.pval, e[1]), what + (g, e)
    elif nR is None or not e[3] or _defined(nR, k):
        assert _near(g.stat, e[0]) and (_near(g.pval, e[1]) or abs(g.pval - e[1]) < PTOL), what + (g, e)
    else:
        assert np.isnan(g.stat) or abs(g.stat) <= 1.0, what + (g, e)
        assert nR > 3 or (g.pval == 1.0 and e[1] == 1.0), what + (g, e)


def _compare_job(g, e, matrix, what, nR=None, k_first=None):
    """(without a matrix, `_defined` above: a view of at most three rows ends its job at the first test with p = 1 -- everything but
    the statistic is compared; a view of four rows whose first subset holds three variables decides on noise -- power only.
    k_first: size of the first subset of the enumeration, min(max_k, |accepted|))"""
    if not matrix and nR is not None and e["suff_power"] and e["status"] and not _defined(nR, k_first):
        assert g["suff_power"] and g["df"] == 0 and g["status"] in (1, 2), what + (g, e)
        if nR <= 3:
            assert (g["status"], g["num_tests"], g["Zs"], g["pval"]) == (1, 1, e["Zs"], 1.0) == (e["status"], e["num_tests"], e["Zs"], e["pval"]), what + (g, e)
        return
    assert g["status"] == e["status"] and g["num_tests"] == e["num_tests"], what + (g, e)
    if e["status"] == 0:
        return
    assert g["Zs"] == e["Zs"] and g["suff_power"] == e["suff_power"] and g["df"] == 0, what + (g, e)
    if matrix:
        assert _same(g["stat"], e["stat"]) and _pclose(g["pval"], e["pval"]) and g["frac"] == e["frac"], what + (g, e)
    else:
        assert _near(g["stat"], e["stat"]) and (_near(g["pval"], e["pval"]) or abs(g["pval"] - e["pval"]) < PTOL), what + (g, e)


@pytest.mark.parametrize("matrix", [True, False], ids=["matrix", "no_matrix"])
@pytest.mark.parametrize("nmin", [NMIN, 0])
@pytest.mark.parametrize("n", sorted(TB.SIZES))
def test_staircase_tests_and_jobs(n, nmin, matrix):
    """fznz_submat_kernel + fznz_single_kernel + the LOCAL segment kernels (matrix path) or fznz_partialcor64 and the fw_fzs.hip
    kernels (recursive_pcor = False) on views of 0 1 2 3 4 19 20 21 63 64 65 127 128 129 n rows, k = 0 .. 3 and lists of 0 1 2 3 6 7 14
    15 variables (m = 2 .. 17): the tree form at n = 130 and 16 384 (W = 256, row 16 383 in the 16-bit list), the sequential form at
    16 385; with n_obs_min = 0 the views of 0 .. 4 rows are tested as well."""
    data = TB.staircase(n)
    orc = TB.oracle_of("staircase", n, not matrix)
    what = (n, nmin, "matrix" if matrix else "no matrix")
    eng = _engine(data, nmin=nmin, max_k=3, recursive_pcor=matrix)
    try:
        X, Y, Zs = TB.stair_tests(n)
        rows = {1 + j: s for j, s in enumerate(TB.SIZES[n])}  # rows of the view (0, y)
        got = eng.test_batch(X, Y, Zs)
        npow = 0
        for i, (x, y, z, g) in enumerate(zip(X, Y, Zs, got)):
            e = orc.test(x, y, z, n_obs_min=nmin)
            _compare_test(g, e, matrix, what + (x, y, z), rows[y], len(z))
            if not matrix and e[3] and nmin:
                r, nR = _reference(n)[i]
                assert nR >= nmin and _near(g.stat, r), what + (x, y, z, g.stat, r)  # the order-free reference
                npow += 1
        assert matrix or not nmin or npow >= 24
        T, C, A = TB.stair_jobs(n)
        jobs = eng.test_subsets_batch(T, C, A)
        for t, c, a, g in zip(T, C, A, jobs):
            _compare_job(g, orc.test_subsets(t, c, a, max_k=3, alpha=0.01, n_obs_min=nmin), matrix, what + (t, c, tuple(a)), rows[c], min(3, len(a)))
        # the pair statistic of a univariate job (the sequential pair form, rec->rxy) is level 0's, to the bit
        nb = eng.pw_univar_neighbors()
        lo, hi = int(nb["off"][0]), int(nb["off"][1])
        nbr = {int(v): float(s) for v, s in zip(nb["idx"][lo:hi], nb["stat"][lo:hi])}
        views = [1 + j for j in range(len(TB.SIZES[n])) if 1 + j in nbr]
        assert len(views) >= 4, (what, sorted(nbr))
        for y in views:
            g = eng.test(0, y, ())
            assert np.float64(g.stat).tobytes() == np.float64(nbr[y]).tobytes() and g.suff_power, what + (y, g, nbr[y])
    finally:
        eng.close()


# ---- 3. list-size switches ----

def test_list_size_switches():
    """One batch with |accepted| = 62, 63, 64 (m = 64, 65, 66) and 512, 513 (FW_TAB_A: fz_subsets_seg_kernel<false, true, true> up to
    512, <false, true, false> beyond) next to short lists, then a batch of short lists only (another m_cap, another LDS size), then the
    long batch again.  alpha near 1, max_tests = 3 000: the cap ends the long jobs."""
    data = TB.wide()
    orc = TB.oracle_of("wide", 130)
    long_batch, small_batch = TB.wide_jobs()
    kw = dict(max_k=3, alpha=0.9999, max_tests=3000)
    eng = _engine(data, **kw)
    try:
        for name, (T, C, A) in (("long", long_batch), ("small", small_batch), ("long again", long_batch)):
            got = eng.test_subsets_batch(T, C, A)
            for t, c, a, g in zip(T, C, A, got):
                e = orc.test_subsets(t, c, a, n_obs_min=NMIN, **kw)
                _compare_job(g, e, True, (name, t, c, len(a)))
                assert e["num_tests"] > 0
    finally:
        eng.close()


# ---- 4. networks ----

def _network(data, monkeypatch, driver, ff, max_k=3, route="host", track=False):
    """-> (network, counters) through the host job pool or the device rounds (the knobs are read per call)"""
    if driver == "host pool":
        monkeypatch.setenv("FW_HOST_HITON", "1")
    else:
        monkeypatch.delenv("FW_HOST_HITON", raising=False)
        monkeypatch.setenv("FW_DEV_MIN_TARGETS", "1")
    eng = _engine(data, route, max_k=max_k)
    try:
        net = eng.lgl(feed_forward=ff, round_size=8 if ff else 0, edge_dict=False, track_rejections=track)
        return net, eng.counters()
    finally:
        eng.close()


def _compare_network(got, cn, exp, p, what):
    ge = dict(zip(zip(got["edge_src"].tolist(), got["edge_dst"].tolist()), got["edge_weight"].tolist()))
    assert ge == exp["edges"] and len(ge) > 0, what
    assert np.array_equal(got["pc_off"], exp["pc_off"]) and np.array_equal(got["pc_idx"], exp["pc_idx"]), what
    assert np.array_equal(got["pc_weight"], exp["pc_weight"], equal_nan=True), what
    assert np.allclose(got["pc_pval"], exp["pc_pval"], rtol=PTOL, atol=0.0, equal_nan=True), what
    assert cn["cond_tests_ref"] == exp["n_cond_tests"] and cn["level0_tests"] == p * (p - 1) // 2, what


@functools.lru_cache(maxsize=None)
def _oracle_network(name, n, ff, max_k=3):
    return TB.oracle_of(name, n).learn(max_k=max_k, feed_forward=ff, round_size=8 if ff else 1, n_obs_min=NMIN, threads=4)


@pytest.mark.parametrize("ff", [False, True], ids=["all_targets", "feed_forward_8"])
@pytest.mark.parametrize("n", TB.N_SMALL + TB.N_LARGE)
def test_chain_networks_on_both_drivers(n, ff, monkeypatch):
    """The whole path -- level 0, sub-matrices, LOCAL segment kernels, HITON-PC -- at every n, through the host job pool and the device
    rounds: edges, weights and directed lists equal the oracle's, p-values within 1e-12, the reference-order test count equal."""
    data = TB.chain(n)
    exp = _oracle_network("chain", n, ff)
    launches = {}
    for driver in ("host pool", "device rounds"):
        got, cn = _network(data, monkeypatch, driver, ff)
        _compare_network(got, cn, exp, 16, (n, ff, driver))
        launches[driver] = cn["kernel_launches"]
    assert launches["host pool"] != launches["device rounds"], launches  # the two drivers really are different paths


def test_hub_network_on_the_device_rounds(monkeypatch):
    """Accepted lists of more than 62 variables on the device rounds (jobs of more than FZNZ_DEV_SMALL = 64 variables: the long-list
    launch, m_lo = 64) against the oracle directly."""
    data = TB.hub()
    exp = _oracle_network("hub", 130, True)
    got, cn = _network(data, monkeypatch, "device rounds", True, track=True)
    _compare_network(got, cn, exp, data.shape[1], ("hub",))
    longest = int(got["rejection_records"]["n_acc"].max())
    assert longest + 2 > 64, longest


@pytest.mark.parametrize("table, n", [("chain", 129), ("staircase", 130)])
@pytest.mark.parametrize("driver", ["host pool", "device rounds"])
def test_max_k_5_networks(table, n, driver, monkeypatch):
    """fz_subsets_seg_kernel<true, true, false> against the oracle: `chain` at n = 129, whose lists hold at most three variables, and
    the staircase table, whose common factor gives lists that subsets of four and five variables are drawn from."""
    data = TB.TABLES[table](n)
    exp = _oracle_network(table, n, False, 5)
    got, cn = _network(data, monkeypatch, driver, False, max_k=5)
    _compare_network(got, cn, exp, data.shape[1], (table, n, driver))


# ---- 5. the NaN directed column on the matrix path ----

def test_constant_column_in_a_view_on_the_matrix_path():
    """A conditioning variable that is absent in every row of a job's view: a zero sum of squares, 0 / 0, and the matrix path stores a
    correlation of 0 for it (cor_subset!), so the enumeration goes on with finite statistics -- where the no-matrix path stops with a
    NaN (tests/test_gpu_fznz.py::test_no_matrix_constant_column_in_a_view)."""
    data, T, Cn, z, (a, b, c, d) = TB.nan_directed()
    orc = TB.oracle_of("nan", 65)
    eng = _engine(data, max_k=3, alpha=0.9999)
    try:
        jobs = [[z], [a, z], [z, a, b], [a, b, c, z], [a, z, b, c, d]]
        got = eng.test_subsets_batch([T] * len(jobs), [Cn] * len(jobs), jobs)
        for acc, g in zip(jobs, got):
            e = orc.test_subsets(T, Cn, acc, max_k=3, alpha=0.9999, n_obs_min=NMIN)
            _compare_job(g, e, True, (tuple(acc),))
            assert np.isfinite(g["stat"]) and np.isfinite(g["pval"]) and g["num_tests"] >= 1
        zs = [(z,), (a, z), (z, a, b), (a, b, z)]
        for zz, g in zip(zs, eng.test_batch([T] * len(zs), [Cn] * len(zs), zs)):
            e = orc.test(T, Cn, zz, n_obs_min=NMIN)
            _compare_test(g, e, True, (zz,))
            assert g.suff_power and np.isfinite(g.stat) and np.isfinite(g.pval)
    finally:
        eng.close()
