"""Sample-count edges of the discrete (mi / mi_nz) kernels against the CPU oracle, through the C ABI.

The discrete path picks its kernel form from the sample count n, and every form masks the last partial word of a column on its own
(DESIGN.md section 2 lists the switches with the test below that crosses each).  The tables here are tiny (12 or 16 variables, one
of 130) and sit ON and NEXT TO every switch: a mask that drops or double-counts the last rows moves a count by one, which the
comparisons of tests/test_gpu_mi.py catch -- df, suff_power, status, num_tests, Zs, CSR lists and test counts equal, statistics and
weights 1e-12 relative, p-values 1e-10 relative -- but only at the shapes a test visits.

Conditions asserted below, so that no comparison is vacuous; the figures are the oracle's alone (CPU), with these generators and
the 240 jobs of `_jobs`, hps = 1, n_obs_min = 0.  Share of tests with suff_power, by size k of the conditioning set:

  dependent, sparse rules    mi  k=0   k=1   k=2   k=3      mi_nz  k=0   k=1   k=2   k=3
  n = 31                       1.00  1.00  0.35  0.00         1.00  0.98  0.02  0.00
  n = 32                       1.00  1.00  0.32  0.05         1.00  0.97  0.00  0.00
  n = 33                       1.00  1.00  0.38  0.00         1.00  1.00  0.02  0.00
  n = 63                       1.00  1.00  0.98  0.18         1.00  1.00  0.27  0.00
  n = 64                       1.00  1.00  0.98  0.13         1.00  1.00  0.32  0.00
  n = 65                       1.00  1.00  0.98  0.17         1.00  1.00  0.47  0.00
  n = 257                      1.00  1.00  1.00  1.00         1.00  1.00  1.00  0.97
  n = 263                      1.00  1.00  1.00  1.00         1.00  1.00  1.00  1.00
  every n in N_EDGE, N_WIDE     1.00  1.00  1.00  1.00         1.00  1.00  1.00  1.00

  dependent, dense rules     mi  k=0   k=1   k=2   k=3      mi_nz  k=0   k=1   k=2   k=3
  n = 31                       1.00  1.00  0.35  0.00         1.00  0.98  0.00  0.00
  n = 32                       1.00  1.00  0.32  0.05         1.00  0.97  0.00  0.00
  n = 33                       1.00  1.00  0.38  0.00         1.00  1.00  0.00  0.00
  n = 63                       1.00  1.00  0.98  0.18         1.00  1.00  0.20  0.00
  n = 64                       1.00  1.00  0.98  0.13         1.00  1.00  0.28  0.00
  n = 65                       1.00  1.00  0.98  0.17         1.00  1.00  0.42  0.00
  n = 257                      1.00  1.00  1.00  1.00         1.00  1.00  1.00  0.93
  n = 263                      1.00  1.00  1.00  1.00         1.00  1.00  1.00  1.00
  every n in N_EDGE, N_WIDE     1.00  1.00  1.00  1.00         1.00  1.00  1.00  1.00
  concentrated, front_empty     1.00  1.00  1.00  1.00         1.00  1.00  1.00  1.00   (both rule sets; largest cell of
                                                                                          concentrated: 65 455 rows)

Networks of `chain` (16 variables, feed_forward = False): edges / level-0 pairs / conditional tests of the oracle
  n = 511    max_k = 3       mi   21 /  70 /  218      mi_nz   14 /  70 /  151
  n = 513    max_k = 3       mi   21 /  75 /  233      mi_nz   14 /  71 /  153
  n = 2047   max_k = 3       mi   22 /  80 /  397      mi_nz   14 /  82 /  177
  n = 2048   max_k = 3       mi   22 /  85 /  410      mi_nz   14 /  80 /  174
  n = 2049   max_k = 3       mi   23 /  79 /  404      mi_nz   14 /  81 /  175
  n = 5120   max_k = 3       mi   22 /  96 /  431      mi_nz   14 /  92 /  197
  n = 5121   max_k = 3       mi   22 /  94 /  426      mi_nz   15 /  94 /  210
  n = 6144   max_k = 3       mi   23 / 103 /  465      mi_nz   15 /  94 /  208
  n = 6145   max_k = 3       mi   22 / 102 /  445      mi_nz   16 /  88 /  202
  n = 65535  max_k = 2       mi   22 / 115 / 1255      mi_nz   14 / 100 /  766
  n = 65536  max_k = 2       mi   22 / 115 / 1257      mi_nz   15 / 104 /  788
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flashweave_jl_amd as fw
from oracle import oracle as O
from tests.util import rel

pytestmark = pytest.mark.gpu
STOL, PTOL = 1e-12, 1e-10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "mi_edges_worker.py")

N_SMALL = (31, 32, 33, 63, 64, 65, 257, 263)
N_EDGE = (505, 511, 512, 513, 2047, 2048, 2049, 5119, 5120, 5121, 6143, 6144, 6145)
N_WIDE = (65535, 65536)
N_NET = (511, 513, 2047, 2048, 2049, 5120, 5121, 6144, 6145)
KINDS = ("mi", "mi_nz")
PROBS = (0.3, 0.35, 0.35)


# ---- inputs ----

def _clip(kind, data, every):
    """mi: the columns `every` selects become binary (two- and three-level variables side by side); mi_nz: column 0 only -- a binary
    column is not zero-adjusted."""
    p = data.shape[1]
    cols = [j for j in range(p) if every(j, p)] if kind == "mi" else [0]
    data[:, cols] = np.minimum(data[:, cols], 1)
    return np.ascontiguousarray(data.astype(np.int32))


def dependent(kind, n, p=12, seed=None):
    """Three hidden three-valued columns; column j keeps base[:, j % 3] with probability 0.6, else a fresh draw."""
    rng = np.random.default_rng(1000 + n if seed is None else seed)
    base = rng.integers(0, 3, (n, 3))
    data = np.empty((n, p), dtype=np.int64)
    for j in range(p):
        keep = rng.random(n) < 0.6
        fresh = rng.choice(3, size=n, p=PROBS)
        data[:, j] = np.where(keep, base[:, j % 3], fresh)
    return _clip(kind, data, lambda j, p_: j < p_ // 2)


def chain(kind, n, p=16, seed=None, probs=PROBS):
    """Column j copies column j - 1 except where, with probability 0.3, it draws afresh: conditioning really removes edges."""
    rng = np.random.default_rng(2000 + n if seed is None else seed)
    data = np.empty((n, p), dtype=np.int64)
    data[:, 0] = rng.choice(3, size=n, p=probs)
    for j in range(1, p):
        fresh = rng.choice(3, size=n, p=probs)
        redraw = rng.random(n) < 0.3
        data[:, j] = np.where(redraw, fresh, data[:, j - 1])
    return _clip(kind, data, lambda j, p_: j % 2 == 1)


def concentrated(kind, n=65535, p=12):
    """All ones but 40 random rows per column: one cell holds nearly every row, a stratum total sits at the 16-bit limit."""
    rng = np.random.default_rng(3000 + n)
    data = np.ones((n, p), dtype=np.int64)
    for j in range(p):
        rows = rng.choice(n, size=40, replace=False)
        data[rows, j] = rng.choice(np.array([0, 2]), size=40)
    return _clip(kind, data, lambda j, p_: j < p_ // 2)


def front_empty(kind, n=8192):
    """`dependent` with rows 0 .. 2 047 zeroed: the form estimate of the streaming loop reads those rows alone and sees nothing."""
    data = dependent(kind, n).copy()
    data[:2048, :] = 0
    return np.ascontiguousarray(data)


def wide_chain(kind, n, p=130):
    """`chain` over 130 variables with nine zeros in ten values: the oracle's sparse level 0 pays per non-zero (2 s, not 9 s, for the
    8 385 pairs at 65 535 samples), the kernels count every row whatever it holds."""
    return chain(kind, n, p, probs=(0.9, 0.05, 0.05))


TABLES = {"dependent": dependent, "chain": chain, "wide_chain": wide_chain, "concentrated": concentrated, "front_empty": front_empty}
DIRECTED = (("concentrated", 65535), ("front_empty", 8192))


@functools.lru_cache(maxsize=None)
def table(name, kind, n):
    data = TABLES[name](kind, n)
    data.setflags(write=False)
    return data


def _jobs(p, m=240, seed=7):
    """m single tests (X, Y | Zs), the size of Zs cycling 0, 1, 2, 3."""
    rng = np.random.default_rng(seed)
    X, Y, Zs = [], [], []
    for i in range(m):
        v = rng.choice(p, size=i % 4 + 2, replace=False)
        X.append(int(v[0])); Y.append(int(v[1])); Zs.append(tuple(int(t) for t in v[2:]))
    return X, Y, Zs


def _subset_jobs(p, m=40, seed=8):
    """m test_subsets jobs (T, candidate, pool of 3 .. 8 variables)."""
    rng = np.random.default_rng(seed)
    T, C, A = [], [], []
    for _ in range(m):
        v = rng.choice(p, size=int(rng.integers(3, 9)) + 2, replace=False)
        T.append(int(v[0])); C.append(int(v[1])); A.append([int(t) for t in v[2:]])
    return T, C, A


# ---- the oracle's side: computed once per table, shared, never written to ----

@functools.lru_cache(maxsize=None)
def oracle_of(name, kind, n, dense, max_k=3):
    return O.Oracle(kind, table(name, kind, n), sparse=not dense, max_k=max_k)


@functools.lru_cache(maxsize=None)
def oracle_single(name, kind, n, dense):
    orc = oracle_of(name, kind, n, dense)
    X, Y, Zs = _jobs(orc.p)
    return tuple(orc.test(x, y, z, hps=1, n_obs_min=0) for x, y, z in zip(X, Y, Zs))


def power_shares(exp):
    """Share of the tests with suff_power for k = 0 .. 3 (test i conditions on i % 4 variables)."""
    return [float(np.mean([e[3] for e in exp[k::4]])) for k in range(4)]


def check_power(n, exp, what):
    sh = power_shares(exp)
    if n >= 505:
        assert sh == [1.0] * 4, (what, sh)
    elif n >= 257:
        assert min(sh[:3]) >= 0.95, (what, sh)
    else:
        assert min(sh[:2]) >= 0.85, (what, sh)


def _close(a, b, tol):
    return (a == b) or (np.isnan(a) and np.isnan(b)) or rel(a, b) < tol


def compare_single(got, exp, jobs, what):
    X, Y, Zs = jobs
    for x, y, z, g, e in zip(X, Y, Zs, got, exp):
        assert (g[2], bool(g[3])) == (e[2], e[3]), (what, x, y, z, tuple(g), e)
        assert _close(g[0], e[0], STOL) and _close(g[1], e[1], PTOL), (what, x, y, z, tuple(g), e)


def _engine(kind, data, dense=False, max_k=3, alpha=0.01):
    n, p = data.shape
    eng = fw.Engine(kind, n, p, max_k=max_k, alpha=alpha, hps=1, n_obs_min=0, dense_rules=dense)
    eng.set_data(data)
    return eng


def run_single(name, kind, n, dense):
    """The 240 jobs in one mixed batch (whose largest conditioning set picks the form) and the k <= 1 jobs as a batch of their own."""
    data = table(name, kind, n)
    X, Y, Zs = _jobs(data.shape[1])
    exp = oracle_single(name, kind, n, dense)
    what = (name, kind, n, "dense" if dense else "sparse")
    eng = _engine(kind, data, dense)
    try:
        lv, mv = eng.levels()
        elv, emv = oracle_of(name, kind, n, dense).levels()
        assert np.array_equal(lv, elv) and np.array_equal(mv, emv), what
        got = eng.test_batch(X, Y, Zs)
        compare_single(got, exp, (X, Y, Zs), what + ("mixed",))
        low = [i for i in range(len(X)) if len(Zs[i]) <= 1]
        sub = ([X[i] for i in low], [Y[i] for i in low], [Zs[i] for i in low])
        got1 = eng.test_batch(*sub)
        compare_single(got1, [exp[i] for i in low], sub, what + ("k<=1",))
    finally:
        eng.close()
    return exp


def full_count(m, max_k=3):
    out, c = 0, 1
    for j in range(1, max_k + 1):
        c = c * (m - j + 1) // j
        out += c
    return out


def run_subsets(name, kind, n, dense):
    """40 jobs at alpha = 0.01 (jobs stop where the reference stops) and the first ten at alpha = 0.9999 (nearly every test is
    'significant': whole enumerations).  -> (jobs that stopped early, jobs that ran through every subset)."""
    data = table(name, kind, n)
    orc = oracle_of(name, kind, n, dense)
    T, C, A = _subset_jobs(data.shape[1])
    what = (name, kind, n, "dense" if dense else "sparse")
    nstop = nall = 0
    for alpha, m in ((0.01, len(T)), (0.9999, 10)):
        eng = _engine(kind, data, dense, alpha=alpha)
        try:
            got = eng.test_subsets_batch(T[:m], C[:m], A[:m])
        finally:
            eng.close()
        for t, c, a, g in zip(T, C, A, got):
            e = orc.test_subsets(t, c, a, max_k=3, alpha=alpha, hps=1, n_obs_min=0)
            assert g["status"] == e["status"] and g["num_tests"] == e["num_tests"], (what, alpha, t, c, a, g, e)
            assert g["Zs"] == e["Zs"] and g["df"] == e["df"] and g["suff_power"] == e["suff_power"], (what, alpha, t, c, a, g, e)
            assert _close(g["stat"], e["stat"], STOL) and _close(g["pval"], e["pval"], PTOL), (what, alpha, t, c, a, g, e)
            assert e["num_tests"] <= full_count(len(a))
            nstop += e["status"] == 1 and e["num_tests"] < full_count(len(a))
            nall += e["status"] == 2 and e["num_tests"] == full_count(len(a))
    return nstop, nall


# ---- 1. single tests at every n ----

@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("n", N_SMALL + N_EDGE + N_WIDE)
@pytest.mark.parametrize("kind", KINDS)
def test_single_tests_at_every_n(kind, n, dense):
    """mi_test_batch_kernel: byte form up to 512 samples, register-resident words up to 6 144, the streaming loop beyond, 32-bit
    counts from 65 536 on -- and under the dense rules the separate stratum total, kept in 16 bits up to 65 535."""
    exp = run_single("dependent", kind, n, dense)
    check_power(n, exp, (kind, n, dense))


# ---- 2. test_subsets at every n ----

@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("n", N_EDGE + N_WIDE)
@pytest.mark.parametrize("kind", KINDS)
def test_test_subsets_at_every_n(kind, n, dense):
    """mi_subsets_seg_kernel (the form is picked from n and the engine's max_k): status, reference-order test count, conditioning
    set, df, statistic, p-value; jobs that stop early and jobs that run through every subset both occur."""
    nstop, nall = run_subsets("dependent", kind, n, dense)
    assert nstop >= 1 and nall >= 1, (nstop, nall)


# ---- 3. directed tables ----

@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
@pytest.mark.parametrize("name,n", DIRECTED)
@pytest.mark.parametrize("kind", KINDS)
def test_directed_tables(kind, name, n, dense):
    """concentrated: a cell of more than 65 000 rows next to near-empty packed neighbours, stratum totals at 0xFFFF.  front_empty: the
    rows the streaming loop's form estimate reads hold nothing, the real rows come later."""
    if name == "concentrated":
        tab, _ = oracle_of(name, kind, n, dense).contingency_table(6, 7)
        assert tab.max() >= 65000, tab.max()
        assert table(name, kind, n).shape[0] == 65535
    else:
        assert not table(name, kind, n)[:2048].any() and table(name, kind, n)[2048:].any(axis=0).all()
    check_power(n, run_single(name, kind, n, dense), (name, kind, dense))
    run_subsets(name, kind, n, dense)


# ---- 4. level 0 ----

def _level0(kind, data, monkeypatch, knob, csc=False):
    n, p = data.shape
    monkeypatch.setenv("FW_L0_MFMA", knob)
    eng = fw.Engine(kind, n, p, max_k=3, hps=1, n_obs_min=0)
    try:
        eng.set_data(O.dense_to_csc(data) if csc else data)
        nb = eng.pw_univar_neighbors()
        return nb, eng.levels(), eng.counters()["level0_tests"]
    finally:
        eng.close()


def check_level0(kind, n, name, monkeypatch):
    data = table(name, kind, n)
    p = data.shape[1]
    exp = oracle_of(name, kind, n, False).level0(alpha=0.01, hps=1, n_obs_min=0)
    assert len(exp["idx"]) > 0
    res = {}
    for knob in ("0", "2"):  # popcount form; matrix-core form wherever it is defined (it is not from 65 536 samples on)
        nb, lv, nt = _level0(kind, data, monkeypatch, knob)
        what = (kind, n, p, "FW_L0_MFMA=" + knob)
        assert np.array_equal(nb["off"], exp["off"]) and np.array_equal(nb["idx"], exp["idx"]), what
        assert np.allclose(nb["stat"], exp["stat"], rtol=STOL, atol=0), what
        assert np.allclose(nb["pval"], exp["pval"], rtol=PTOL, atol=0), what
        assert nt == p * (p - 1) // 2, what
        res[knob] = (nb, lv)
    for f in ("off", "idx", "stat", "pval"):
        assert res["0"][0][f].tobytes() == res["2"][0][f].tobytes(), (kind, n, p, f)
    nb, lv, nt = _level0(kind, data, monkeypatch, "0", csc=True)  # the other upload route builds the planes' tails itself
    for a, b in zip(lv, res["0"][1]):
        assert np.array_equal(a, b), (kind, n, p, "levels, CSC upload")
    for f in ("off", "idx", "stat", "pval"):
        assert nb[f].tobytes() == res["0"][0][f].tobytes(), (kind, n, p, f, "CSC upload")
    assert nt == p * (p - 1) // 2


@pytest.mark.parametrize("n", (63, 64, 65) + N_EDGE + N_WIDE)
@pytest.mark.parametrize("kind", KINDS)
def test_level0_at_every_n(kind, n, monkeypatch):
    """mi_level0_* on 64-sample words and 8-word stages: popcount and matrix-core form against the oracle and each other, dense and
    CSC upload."""
    check_level0(kind, n, "chain", monkeypatch)


@pytest.mark.parametrize("n", (511, 513, 65535))
@pytest.mark.parametrize("kind", KINDS)
def test_level0_two_tiles(kind, n, monkeypatch):
    """130 variables: two 128-wide tiles of the matrix-core form, the second ragged."""
    check_level0(kind, n, "wide_chain", monkeypatch)


# ---- 5. / 6. networks, and knobs the library reads once per process (through the worker) ----

def network_result(kind, n, max_k):
    """One `chain` network of the engine, in plain lists (the worker prints them as JSON)."""
    data = table("chain", kind, n)
    eng = fw.Engine(kind, n, data.shape[1], max_k=max_k)
    try:
        eng.set_data(data)
        net = eng.lgl(feed_forward=False, round_size=0)
        cn = eng.counters()
    finally:
        eng.close()
    edges = sorted(net["edges"])
    return dict(edges=[list(e) for e in edges], edge_weight=[net["edges"][e] for e in edges], pc_off=net["pc_off"].tolist(),
                pc_idx=net["pc_idx"].tolist(), pc_weight=net["pc_weight"].tolist(), cond_tests_ref=int(cn["cond_tests_ref"]),
                level0_tests=int(cn["level0_tests"]))


def single_result(kind, n, dense):
    """The 240 single tests on `dependent`, in plain lists."""
    data = table("dependent", kind, n)
    eng = _engine(kind, data, dense)
    try:
        got = eng.test_batch(*_jobs(data.shape[1]))
    finally:
        eng.close()
    return [[g.stat, g.pval, int(g.df), int(g.suff_power)] for g in got]


WORKER_KNOBS = ("FW_MI_ROW4", "FW_MI_ROWK", "FW_HOST_HITON", "FW_DEV_MIN_TARGETS", "FW_L0_MFMA")


def run_worker(mode, kinds, ns, max_k=3, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in WORKER_KNOBS}
    env.update({k: str(v) for k, v in knobs.items()})
    cmd = [sys.executable, WORKER, "--mode", mode, "--kinds", ",".join(kinds), "--ns", ",".join(str(n) for n in ns), "--max-k", str(max_k)]
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@functools.lru_cache(maxsize=None)
def oracle_network(kind, n, max_k):
    """-> (the oracle's network, its number of level-0 pairs); four threads: same results as one (Oracle.learn)."""
    orc = oracle_of("chain", kind, n, False, max_k)
    net = orc.learn(max_k=max_k, feed_forward=False, threads=4)
    l0 = orc.level0(alpha=0.01, hps=5, n_obs_min=orc.auto_n_obs_min(-1, 5, max_k))
    return net, len(l0["idx"]) // 2


def compare_network(got, kind, n, max_k, what):
    exp, pairs = oracle_network(kind, n, max_k)
    # the network is not vacuous: conditioning removed level-0 pairs, and the kernels ran a real number of conditional tests
    assert len(exp["edges"]) < pairs and exp["n_cond_tests"] >= 150, (what, len(exp["edges"]), pairs, exp["n_cond_tests"])
    edges = sorted(exp["edges"])
    assert [tuple(e) for e in got["edges"]] == edges, what
    assert np.allclose(got["edge_weight"], [exp["edges"][e] for e in edges], rtol=1e-11, atol=1e-15, equal_nan=True), what
    assert got["pc_off"] == exp["pc_off"].tolist() and got["pc_idx"] == exp["pc_idx"].tolist(), what
    assert np.allclose(np.array(got["pc_weight"], dtype=np.float64), exp["pc_weight"], rtol=1e-11, atol=1e-15, equal_nan=True), what
    assert got["cond_tests_ref"] == exp["n_cond_tests"], what
    assert got["level0_tests"] == 16 * 15 // 2, what


# FW_MI_ROW4 -> sample counts: 2 (four subsets per step up to 5 120 samples) differs from the default only in (2 048, 5 120]
ROW4_NS = {0: N_NET, 1: N_NET, 2: (2048, 2049, 5120, 5121)}


@pytest.mark.parametrize("row4", sorted(ROW4_NS))
def test_networks_across_form_switches(row4):
    """dh_mi_target_kernel in each of its forms -- four subsets per wavefront step (up to 2 048 samples, or 5 120 when forced) or one;
    register-resident words up to 6 144 samples or the streaming loop: edges, directed lists and the reference-order test count
    equal the oracle's, weights within 1e-11."""
    ns = ROW4_NS[row4]
    out = run_worker("net", KINDS, ns, 3, FW_DEV_MIN_TARGETS=1, FW_MI_ROW4=row4)
    for kind in KINDS:
        for n in ns:
            compare_network(out["%s:%d" % (kind, n)], kind, n, 3, ("FW_MI_ROW4=%d" % row4, kind, n))


@pytest.mark.parametrize("kind", KINDS)
def test_networks_host_pool_across_form_switches(kind, monkeypatch):
    """The same networks through the host job pool over mi_subsets_seg_kernel (FW_HOST_HITON is read per call)."""
    monkeypatch.setenv("FW_HOST_HITON", "1")
    for n in N_NET:
        compare_network(network_result(kind, n, 3), kind, n, 3, ("host pool", kind, n))


@pytest.mark.parametrize("kind", KINDS)
def test_networks_at_the_16_bit_limit(kind, monkeypatch):
    """max_k = 2 (the k = 3 segment path refuses more than 65 535 samples by design): packed 16-bit counts at 65 535 samples, 32-bit
    ones at 65 536, in the persistent kernel and through the host job pool."""
    out = run_worker("net", (kind,), N_WIDE, 2, FW_DEV_MIN_TARGETS=1)
    monkeypatch.setenv("FW_HOST_HITON", "1")
    for n in N_WIDE:
        compare_network(out["%s:%d" % (kind, n)], kind, n, 2, ("persistent kernel", kind, n))
        compare_network(network_result(kind, n, 2), kind, n, 2, ("host pool", kind, n))


def test_popcount_form_only():
    """FW_MI_ROWK=99 keeps the byte and row forms off: the only way to the popcount counting loop on nz-adjusted tables of up to 512
    samples.  Statistics against the oracle, integers against the default run of this process as well."""
    assert "FW_MI_ROWK" not in os.environ
    out = run_worker("single", KINDS, N_EDGE, 3, FW_MI_ROWK=99)
    for kind in KINDS:
        for n in N_EDGE:
            for dense in (False, True):
                jobs = _jobs(table("dependent", kind, n).shape[1])
                got = out["%s:%d:%d" % (kind, n, int(dense))]
                compare_single(got, oracle_single("dependent", kind, n, dense), jobs, (kind, n, dense, "FW_MI_ROWK=99"))
                dflt = single_result(kind, n, dense)
                assert [g[2:] for g in got] == [d[2:] for d in dflt], (kind, n, dense)
