"""The matrix-free Fisher-z kernels (fw_fzs.hip: fzs_colstat_kernel, fzs_test_batch_kernel, fzs_subsets_seg_kernel, fzs_gram_kernel;
learn_network(recursive_pcor=False)) on and next to every point where the sample count, the list length or the form switch the code
path, against the CPU oracle, through Engine.  DESIGN.md section 4.7 lists the switches with the test below that crosses each;
tests/test_fzs_edges_cpu.py asserts on the oracle alone that no comparison here is vacuous and pins the oracle's `pcor` path to a
numpy.longdouble reference (1e-12, on the offset tables too).

Tolerances are those of tests/test_gpu_fzs.py: 1e-11 absolute on the statistic, 1e-8 relative on p; status, num_tests, conditioning
sets, power and test counts are equal; two NaNs are equal, and p is compared wherever it is defined.  The Gram form and the streamed
form of the segment kernel agree with each other within 1e-12.  Univariate tests stay bit-exact against the Float32 matrix.
n_obs_min is passed explicitly, the same value to the engine and to the oracle."""
import numpy as np
import pytest

import flashweave_jl_amd as fw
from oracle import oracle as O
from tests import fzs_edges_tables as TB

pytestmark = pytest.mark.gpu
NMIN = TB.N_OBS_MIN
STOL, PTOL, FORMS_TOL = 1e-11, 1e-8, 1e-12
FORMS = (("gram", "1"), ("streamed", "0"))  # FW_FZS_GRAM, read per launch


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def _stat_ok(a, b, tol=STOL):
    return _same(a, b) or abs(a - b) < tol


def _p_ok(a, b, tol=PTOL):
    return _same(a, b) or abs(a - b) <= tol * max(abs(b), 1e-300) + 1e-300


def _dev(a, b):
    return 0.0 if _same(a, b) else abs(a - b)


def _engine(data, **kw):
    n, p = data.shape
    kw.setdefault("max_k", 3)
    eng = fw.Engine("fz", n, p, recursive_pcor=False, n_obs_min=NMIN, **kw)
    try:
        eng.set_data(data)
    except Exception:
        eng.close()
        raise
    return eng


def _check_tests(got, exp, tests, what, univariate=None):
    """got: TestResult list; exp: oracle tuples.  Collects every miss, prints the worst deviation, then asserts."""
    bad, worst = [], 0.0
    for x, y, z, g, e in zip(*tests, got, exp):
        ok = g.suff_power == e[3] and g.df == 0
        if len(z) == 0 and univariate is not None:
            ok = ok and g.stat == float(univariate[x, y]) and g.stat == e[0] and _p_ok(g.pval, e[1])
        else:
            ok = ok and _stat_ok(g.stat, e[0]) and _p_ok(g.pval, e[1])
            worst = max(worst, _dev(g.stat, e[0]))
        if not ok:
            bad.append((x, y, z, g, e))
    print(what, "worst deviation of the statistic %.2e over %d tests" % (worst, len(got)))
    assert not bad, (what, len(bad), bad[:3])
    return worst


def _check_jobs(got, exp, jobs, what, tol=STOL, ptol=PTOL):
    bad, worst = [], 0.0
    for t, c, a, g, e in zip(*jobs, got, exp):
        ok = (g["status"], g["num_tests"], g["Zs"], g["suff_power"]) == (e["status"], e["num_tests"], e["Zs"], e["suff_power"]) and g["df"] == 0
        ok = ok and _stat_ok(g["stat"], e["stat"], tol) and _p_ok(g["pval"], e["pval"], ptol)
        worst = max(worst, _dev(g["stat"], e["stat"]))
        if not ok:
            bad.append((t, c, len(a), g, e))
    print(what, "worst deviation of the statistic %.2e over %d jobs" % (worst, len(got)))
    assert not bad, (what, len(bad), bad[:3])
    return worst


def _jobs_in_forms(data, jobs, monkeypatch, **kw):
    """-> {"gram": results, "streamed": results}: the same batch through fzs_gram_kernel + fzs_subsets_seg_kernel<., 0, true> and
    through the streamed form (<., 8, false> where fzs_hold_xy holds: n % 4 == 0 and n <= 2048; <., 0, false> elsewhere)"""
    res = {}
    for form, knob in FORMS:
        monkeypatch.setenv("FW_FZS_GRAM", knob)
        eng = _engine(data, **kw)
        try:
            res[form] = eng.test_subsets_batch(*jobs)
        finally:
            eng.close()
    return res


def _check_forms(res, exp, jobs, what):
    _check_jobs(res["gram"], res["streamed"], jobs, what + ("gram against streamed",), FORMS_TOL, 1e-9)
    for form, _ in FORMS:
        _check_jobs(res[form], exp, jobs, what + (form,))


# ---- 1. single tests at every n ----

@pytest.mark.parametrize("n", TB.N_ALL)
def test_single_tests_at_every_n(n):
    """fzs_test_batch_kernel<5, T> with k = 0 .. 5 mixed, then <3, T> with k <= 3; T = 8 where n % 4 == 0 and n <= 2048 (X / Y in LDS,
    16-byte rows: whole 256-sample rows at 256 and 2048, a partial last row elsewhere, no full row at 60 .. 68), T = 0 elsewhere (4-byte
    loads, 64-sample steps; 63 / 64 / 65: one step, one step exactly, two).  47 and 31 tests: the last workgroup holds three."""
    data = TB.centred(n, TB.P_SINGLE)
    eng = _engine(data, max_k=5)
    try:
        cm = eng.cor()
        orc = O.Oracle("fz", cor_mat=cm, n_obs=n)
        orc.set_fz_data(data.astype(np.float64))
        for tests in (TB.single_tests(), TB.single_tests(kmax=3, count=31, seed=2)):
            got = eng.test_batch(*tests)
            exp = [orc.test(x, y, z, n_obs_min=NMIN) for x, y, z in zip(*tests)]
            _check_tests(got, exp, tests, (n, max(len(z) for z in tests[2])), univariate=cm)
        orc.close()
    finally:
        eng.close()


# ---- 2. test_subsets at every n, in all three segment forms ----

@pytest.mark.parametrize("max_k", [3, 5])
@pytest.mark.parametrize("n", TB.N_ALL)
def test_subsets_at_every_n_in_every_form(n, max_k, monkeypatch):
    """Lists of 9 (129 / 381 subsets of 3 / 5 sizes): some jobs stop at rank 0, 2 or 6, the others run through every run of 16 ranks,
    several sweeps of the four wavefronts and every change of subset size; the enumeration ends inside a group."""
    data = TB.centred(n, TB.P_SINGLE)
    orc = TB.oracle_of("centred", n, TB.P_SINGLE, cor="eye")
    jobs = TB.nine_jobs()
    exp = [orc.test_subsets(t, c, a, max_k=max_k, alpha=0.01, n_obs_min=NMIN) for t, c, a in zip(*jobs)]
    _check_forms(_jobs_in_forms(data, jobs, monkeypatch, max_k=max_k), exp, jobs, (n, max_k))


# ---- 3. list lengths ----

@pytest.mark.parametrize("n", TB.N_LISTS)
def test_list_lengths_in_both_forms(n, monkeypatch):
    """|accepted| = 1 2 3 6 10 14 77 78 79 80: m = a + 2 on both sides of a multiple of 4 (the clamped 4 x 4 tiles of fzs_gram_kernel)
    and of 80 (the job's matrix in LDS, through L2 beyond; one launch holds both, lds_m = 80).  alpha near 1; the long jobs end at the
    cap, whose last rank is the second of a group of four, the short ones enumerate 1 .. 469 subsets and end inside a group."""
    data = TB.centred(n, TB.P_LISTS)
    orc = TB.oracle_of("centred", n, TB.P_LISTS, cor="eye")
    jobs = TB.list_jobs()
    kw = dict(max_k=3, alpha=TB.LIST_ALPHA, max_tests=TB.LIST_CAP)
    exp = [orc.test_subsets(t, c, a, n_obs_min=NMIN, **kw) for t, c, a in zip(*jobs)]
    _check_forms(_jobs_in_forms(data, jobs, monkeypatch, **kw), exp, jobs, (n, "lists"))
    # short lists alone: lds_m = 16, every matrix in LDS
    short = tuple(v[:12] for v in jobs)
    _check_forms(_jobs_in_forms(data, short, monkeypatch, **kw), exp[:12], short, (n, "short lists"))


@pytest.mark.parametrize("cap", TB.CAPS_IN_GROUP)
def test_cap_inside_a_group(cap, monkeypatch):
    """max_tests = 3001, 3002, 3003: the capped test is the first, second, third of its group of four (K = 3: G = 4)"""
    n = TB.N_LISTS[1]
    data = TB.centred(n, TB.P_LISTS)
    orc = TB.oracle_of("centred", n, TB.P_LISTS, cor="eye")
    jobs = tuple(v[-4:] for v in TB.list_jobs())
    kw = dict(max_k=3, alpha=TB.LIST_ALPHA, max_tests=cap)
    exp = [orc.test_subsets(t, c, a, n_obs_min=NMIN, **kw) for t, c, a in zip(*jobs)]
    assert all(e["num_tests"] == cap for e in exp)
    _check_forms(_jobs_in_forms(data, jobs, monkeypatch, **kw), exp, jobs, (n, "cap", cap))


# ---- 4. networks ----

@pytest.mark.parametrize("n", TB.N_NET)
def test_networks(n):
    """lgl on centred(n, 40), all targets at once and feed-forward rounds of 8: edges, weights (1e-11) and the reference-order test
    count against the oracle; at n = 255 and 2049 without any correlation matrix as well (dense_cor = False), edge for edge the
    network of dense_cor = True."""
    data = TB.centred(n, TB.P_NET)
    eng = _engine(data)
    e2 = _engine(data, dense_cor=False) if n in TB.N_NET_NO_MATRIX else None
    try:
        cm = eng.cor()
        orc = O.Oracle("fz", cor_mat=cm, n_obs=n)
        orc.set_fz_data(data.astype(np.float64))
        for ff, rs in ((False, 0), (True, 8)):
            eng.reset_counters()
            net = eng.lgl(feed_forward=ff, round_size=rs)
            exp = orc.learn(max_k=3, feed_forward=ff, round_size=rs if ff else 1, n_obs_min=NMIN)
            assert set(net["edges"]) == set(exp["edges"]) and len(exp["edges"]) > 20, (n, ff, len(net["edges"]), len(exp["edges"]))
            worst = max(abs(net["edges"][k] - w) for k, w in exp["edges"].items())
            print(n, ff, "edges %d, worst weight deviation %.2e" % (len(exp["edges"]), worst))
            assert worst < STOL
            assert eng.counters()["cond_tests_ref"] == exp["n_cond_tests"]
            if e2 is not None:
                assert e2.lgl(feed_forward=ff, round_size=rs)["edges"] == net["edges"]
        orc.close()
    finally:
        eng.close()
        if e2 is not None:
            e2.close()


# ---- 5. degenerate columns ----

@pytest.mark.parametrize("n", TB.N_LISTS)
def test_degenerate_columns(n, monkeypatch):
    """A constant column, the exact copy of a column, a variable listed twice -- in explicit tests (T = 8 at n = 64, T = 0 at 257) and in
    accepted lists, both segment forms.  The device returns what the oracle returns (tests/test_fzs_edges_cpu.py pins that).  Kind
    "0/0": a step of the recursion is 0 / 0 in exact arithmetic (a zero sum of squares, or a correlation of exactly 1 conditioned on);
    StatsBase.partialcor forms the identical sums of identical columns, gets 1 exactly and returns NaN, as the oracle does, and
    NaN < alpha is false: the job stops there.  For these NaN-ness, p and suff_power are compared; for kind "value" (the twin of a
    column that is neither X nor Y) the statistic at 1e-11."""
    data = TB.degenerate(n)
    orc = TB.oracle_of("degenerate", n, TB.P_SINGLE, cor="eye")
    tests = tuple(list(v) for v in zip(*[(x, y, z) for _, x, y, z, _ in TB.DEGENERATE_TESTS]))
    eng = _engine(data)
    try:
        got = eng.test_batch(*tests)
    finally:
        eng.close()
    bad = []
    for (name, x, y, z, kind), g in zip(TB.DEGENERATE_TESTS, got):
        e = orc.test(x, y, z, n_obs_min=NMIN)
        print(n, name, "device", (g.stat, g.pval), "oracle", e[:2])
        ok = g.suff_power == e[3] and np.isnan(g.stat) == np.isnan(e[0]) and _p_ok(g.pval, e[1])
        if kind == "value":
            ok = ok and _stat_ok(g.stat, e[0])
        if not ok:
            bad.append((name, g, e))
    jobs = tuple(list(v) for v in zip(*[(t, c, list(a)) for _, t, c, a in TB.DEGENERATE_JOBS]))
    exp = [orc.test_subsets(t, c, a, max_k=3, alpha=0.01, n_obs_min=NMIN) for t, c, a in zip(*jobs)]
    res = _jobs_in_forms(data, jobs, monkeypatch)
    for form, _ in FORMS:
        for (name, _, _, _), g, e in zip(TB.DEGENERATE_JOBS, res[form], exp):
            print(n, form, name, "device", (g["status"], g["num_tests"], g["Zs"], g["stat"], g["pval"]), "oracle", (e["status"], e["num_tests"], e["Zs"], e["stat"], e["pval"]))
            ok = (g["status"], g["num_tests"], g["Zs"], g["suff_power"]) == (e["status"], e["num_tests"], e["Zs"], e["suff_power"])
            ok = ok and np.isnan(g["stat"]) == np.isnan(e["stat"]) and _p_ok(g["pval"], e["pval"])
            if np.isfinite(e["stat"]):
                ok = ok and _stat_ok(g["stat"], e["stat"])
            if not ok:
                bad.append((form, name, g, e))
    assert not bad, (n, len(bad), bad)


# ---- 6. offset columns ----

@pytest.mark.parametrize("n", TB.N_OFFSET)
@pytest.mark.parametrize("ratio", TB.RATIOS)
def test_offset_columns(ratio, n, monkeypatch):
    """Columns at ratio * sigma (30, 1 000, 30 000): a table passed with normalize=False is legitimate input.  Explicit tests with
    k = 1 .. 3 (T = 0 at n = 255, T = 8 at n = 2000) and lists of 9 in both segment forms, at the tolerance of the centred tables: the
    oracle is within 1.4e-14 of the long-double reference here (tests/test_fzs_edges_cpu.py)."""
    data = TB.offset(n, TB.P_SINGLE, 0, ratio)
    orc = TB.oracle_of("offset", n, TB.P_SINGLE, ratio, cor="eye")
    tests = TB.offset_tests()
    eng = _engine(data)
    try:
        got = eng.test_batch(*tests)
    finally:
        eng.close()
    exp = [orc.test(x, y, z, n_obs_min=NMIN) for x, y, z in zip(*tests)]
    jobs = TB.nine_jobs()
    expj = [orc.test_subsets(t, c, a, max_k=3, alpha=0.01, n_obs_min=NMIN) for t, c, a in zip(*jobs)]
    res = _jobs_in_forms(data, jobs, monkeypatch)
    what = ("offset", ratio, n)
    worst = {}
    for form, _ in FORMS:  # measured before anything is asserted
        worst[form] = max(_dev(g["stat"], e["stat"]) for g, e in zip(res[form], expj))
    print(what, "explicit %.2e, gram %.2e, streamed %.2e" % (max(_dev(g.stat, e[0]) for g, e in zip(got, exp)), worst["gram"], worst["streamed"]))
    _check_tests(got, exp, tests, what)
    _check_forms(res, expj, jobs, what)


@pytest.mark.parametrize("n", TB.N_OFFSET)
def test_offset_columns_fz_nz_without_a_matrix(n, monkeypatch):
    """The same table (no zeros: every view holds every row) through fznz_submat_kernel's Float64 view matrices (recursive_pcor = False
    on fz_nz data) at ratio 1 000: that kernel centres both factors, so the offset does not reach its sums."""
    data = TB.offset(n, TB.P_SINGLE, 0, 1000)
    assert (data != 0).all()
    orc = O.Oracle("fz_nz", data=data.astype(np.float64))
    orc.set_fz_nz_stream(True)
    eng = fw.Engine("fz_nz", n, TB.P_SINGLE, max_k=3, recursive_pcor=False, n_obs_min=NMIN)
    try:
        eng.set_data(data)
        tests = TB.offset_tests()
        got = eng.test_batch(*tests)
        _check_tests(got, [orc.test(x, y, z, n_obs_min=NMIN) for x, y, z in zip(*tests)], tests, ("fz_nz offset", n))
        jobs = TB.nine_jobs()
        exp = [orc.test_subsets(t, c, a, max_k=3, alpha=0.01, n_obs_min=NMIN) for t, c, a in zip(*jobs)]
        _check_jobs(eng.test_subsets_batch(*jobs), exp, jobs, ("fz_nz offset jobs", n))
    finally:
        eng.close()
        orc.close()
