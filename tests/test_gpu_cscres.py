"""CSC-resident fz_nz layout (fw_set_data_csc_f32_resident, learn_network(csc_resident=True)) against the dense-resident layout of
the same library, which tests/test_gpu_fznz.py and the goldens pin to the oracle: every comparison is exact -- == on lists and
sets, tobytes() on weights, statistics and p-values -- because the two layouts run the same kernels over the same rows in the same
order and differ only in how one value is loaded.  One network is also compared with the oracle directly.

Table A (130 x 37): a partial last plane word, p no multiple of the 16 x 16 level-0 tile, an all-zero column, a column without a
zero, columns whose only value sits in row 63 / 64 / 129, stored 0.0f entries in the triple.  Table B (16 448 x 12, ~5 % fill):
n > FZNZ_ROWS_LDS and W = 257 > 256, the sequential branch of fznz_submat_kernel.  Hub table (130 x 110): one variable that every
other one depends on, so that its accepted list passes 62 entries -- jobs of more than FZNZ_DEV_SMALL = 64 variables, the long-list
launch of the device rounds (no job of table A can reach that size: it has 37 variables)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import io as fio
from oracle import oracle as O
from tests.util import GOLDEN, ROOT, read_edgelist

pytestmark = pytest.mark.gpu

NET_KEYS = ("pc_off", "pc_idx", "pc_weight", "pc_pval", "edge_src", "edge_dst", "edge_weight")


def _triple(dense, stored_zero=None):
    """CSC triple of a dense Float32 matrix: an entry per value != 0, plus an explicit 0.0f entry wherever stored_zero is set."""
    keep = dense != 0
    if stored_zero is not None:
        keep = keep | stored_zero
    colptr = np.concatenate([[0], np.cumsum(keep.sum(axis=0))]).astype(np.int64)
    rows = np.concatenate([np.nonzero(keep[:, c])[0] for c in range(dense.shape[1])]).astype(np.int32)
    vals = np.concatenate([dense[keep[:, c], c] for c in range(dense.shape[1])]).astype(np.float32)
    return colptr, rows, vals


def _factor_table(n, p, fill, seed, strength):
    """clr_nz-like values: a common factor (so that conditional tests happen) plus noise, present with probability `fill`."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, 1))
    sign = np.where(rng.random(p) < 0.5, -1.0, 1.0)
    x = 2.0 + strength * f * sign + (1.0 - 0.5 * strength) * rng.standard_normal((n, p))
    x = np.where(rng.random((n, p)) < fill, x, 0.0).astype(np.float32)
    return x


@pytest.fixture(scope="module")
def table_a():
    n, p = 130, 37
    x = _factor_table(n, p, 0.85, 1, 0.9)
    x[:, 0] = 0.0
    x[:, 1] = np.where(x[:, 1] == 0, np.float32(1.25), x[:, 1])  # non-zero in every row
    for c, row in ((2, 63), (3, 64), (4, 129)):
        x[:, c] = 0.0
        x[row, c] = 3.5
    rng = np.random.default_rng(2)
    stored_zero = (x == 0) & (rng.random((n, p)) < 0.3)  # absences the triple stores as 0.0f
    stored_zero[:, 0] = False
    stored_zero[5, 0] = True  # the all-zero column holds one stored zero
    x = np.asfortranarray(x)
    triple = _triple(x, stored_zero)
    assert np.count_nonzero(triple[2] == 0) > 100 and (x[:, 1] != 0).all() and not x[:, 0].any()
    return dict(n=n, p=p, dense=x, triple=triple, nnz=int(np.count_nonzero(x)))


@pytest.fixture(scope="module")
def table_b():
    n, p = 16448, 12
    x = np.asfortranarray(_factor_table(n, p, 0.05, 3, 0.9))
    return dict(n=n, p=p, dense=x, triple=_triple(x), nnz=int(np.count_nonzero(x)))


@pytest.fixture(scope="module")
def table_hub():
    """Variable 0 is the hub, every other one a noisy copy of it (independent of each other given the hub, so nothing screens them
    off from it: the hub's accepted list grows past 62); variables 100 .. 103 are means of two copies each, independent of the hub
    given both, so rejections happen against long lists.  8 % of the ordinary cells are absent, a third of those stored as 0.0f."""
    n, p = 130, 110
    rng = np.random.default_rng(11)
    h = rng.standard_normal(n)
    x = 2.0 + 0.9 * h[:, None] + 0.55 * rng.standard_normal((n, p))
    x[:, 0] = 2.0 + h
    for y, (a, b) in ((100, (1, 2)), (101, (3, 4)), (102, (5, 6)), (103, (7, 8))):
        x[:, y] = 0.5 * (x[:, a] + x[:, b]) + 0.1 * rng.standard_normal(n)
    present = rng.random((n, p)) < 0.92
    present[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 100, 101, 102, 103]] = True
    x = np.asfortranarray(np.where(present, x, 0.0).astype(np.float32))
    stored_zero = (x == 0) & (np.random.default_rng(12).random((n, p)) < 0.33)
    return dict(n=n, p=p, dense=x, triple=_triple(x, stored_zero), nnz=int(np.count_nonzero(x)))


def _engines(t, **kw):
    d = fw.Engine("fz_nz", t["n"], t["p"], **kw)
    d.set_data(t["dense"])
    s = fw.Engine("fz_nz", t["n"], t["p"], **kw)
    s.set_data(t["triple"], csc_resident=True)
    return d, s


def _net_bytes(net):
    out = {k: net[k].tobytes() for k in NET_KEYS}
    if "rejection_records" in net:
        out["rejection_records"] = net["rejection_records"].tobytes()
    return out


def _subsets_bytes(res):
    return [(r["status"], np.array([r["stat"], r["pval"], r["frac"]]).tobytes(), r["df"], r["suff_power"], r["Zs"], r["num_tests"]) for r in res]


def _jobs(p, targets, sizes, seed):
    """Every (T, candidate) pair of the targets, with an accepted set of each size drawn from the other variables."""
    rng = np.random.default_rng(seed)
    T, Cn, A = [], [], []
    for t in targets:
        for c in range(p):
            if c == t:
                continue
            others = [v for v in range(p) if v not in (t, c)]
            for a in sizes:
                if a > len(others):
                    continue
                T.append(t); Cn.append(c); A.append([int(v) for v in rng.choice(others, size=a, replace=False)])
    return T, Cn, A


def test_level0_identical(table_a):
    d, s = _engines(table_a, max_k=3)
    try:
        a, b = d.pw_univar_neighbors(), s.pw_univar_neighbors()
        assert len(a["idx"]) > 0
        for k in ("off", "idx", "stat", "pval"):
            assert a[k].tobytes() == b[k].tobytes(), k
    finally:
        d.close(); s.close()


def test_subsets_identical_over_every_pair_of_some_targets(table_a):
    # targets: the column without a zero, ordinary columns, the single-value columns (views of at most one row) and the zero column
    T, Cn, A = _jobs(table_a["p"], (1, 5, 6, 20, 36, 2, 4, 0), range(0, 6), 7)
    d, s = _engines(table_a, max_k=3)
    try:
        a, b = d.test_subsets_batch(T, Cn, A), s.test_subsets_batch(T, Cn, A)
        assert _subsets_bytes(a) == _subsets_bytes(b)
        assert sum(r["num_tests"] > 0 for r in a) > 100 and {r["status"] for r in a} >= {0, 1}
        # the explicit single tests read the same sub-matrices
        zs = [tuple(z[:3]) for z in A]
        ta, tb = d.test_batch(T, Cn, zs), s.test_batch(T, Cn, zs)
        assert [(np.array([r.stat, r.pval]).tobytes(), r.df, r.suff_power) for r in ta] == [(np.array([r.stat, r.pval]).tobytes(), r.df, r.suff_power) for r in tb]
    finally:
        d.close(); s.close()


@pytest.mark.parametrize("table, round_size, max_k, fast_elim", [
    ("table_a", 1, 3, True), ("table_a", 8, 3, True), ("table_a", 1, 0, True), ("table_a", 1, 5, True), ("table_a", 8, 5, True),
    ("table_a", 1, 3, False), ("table_a", 8, 3, False),
    ("table_hub", 1, 3, True), ("table_hub", 8, 3, True), ("table_hub", 8, 3, False)])
def test_networks_and_rejection_logs_identical(request, table, round_size, max_k, fast_elim, monkeypatch):
    # round_size 1: the host job pool; round_size 8: the device rounds (a test knob lets rounds of 8 targets onto the device).
    # table_a: every job fits the small-LDS launch of the device rounds; table_hub: jobs of more than 64 variables, the long-list launch
    t = request.getfixturevalue(table)
    monkeypatch.setenv("FW_DEV_MIN_TARGETS", "1")
    d, s = _engines(t, max_k=max_k)
    try:
        kw = dict(feed_forward=True, round_size=round_size, fast_elim=fast_elim, track_rejections=True, edge_dict=False)
        a, b = d.lgl(**kw), s.lgl(**kw)
        assert _net_bytes(a) == _net_bytes(b)
        assert len(a["edge_src"]) > 0
        ca, cb = d.counters(), s.counters()
        for k in ("cond_tests_ref", "cond_tests_evaluated", "subsets_calls", "subsets_launches"):
            assert ca[k] == cb[k], k
        assert cb["kernel_launches"] == ca["kernel_launches"] + 3  # (the CSC upload is three launches, the dense upload none)
        longest = int(b["rejection_records"]["n_acc"].max()) if len(b["rejection_records"]) else 0
        print("%s, round_size %d, max_k %d, fast_elim %s: %d edges, %d rejections, %d conditional tests, longest accepted list %d"
              % (table, round_size, max_k, fast_elim, len(a["edge_src"]), len(a["rejection_records"]), ca["cond_tests_ref"], longest))
        if max_k > 0:
            assert ca["cond_tests_ref"] > 0 and len(b["rejection_records"]) > 0
        if table == "table_hub":
            # a candidate was tested, and rejected, against an accepted list of more than 62 variables: that job's sub-matrix has
            # more than FZNZ_DEV_SMALL = 64 variables, which only the long-list launch of a device round computes (m_lo = 64)
            assert longest + 2 > 64
        if round_size == 8 and max_k > 0:
            # the device rounds really ran: the host pool (FW_NZ_DEV=0) launches differently and finds the same network
            monkeypatch.setenv("FW_NZ_DEV", "0")
            h = fw.Engine("fz_nz", t["n"], t["p"], max_k=max_k)
            try:
                h.set_data(t["triple"], csc_resident=True)
                assert _net_bytes(h.lgl(**kw)) == _net_bytes(b)
                assert h.counters()["kernel_launches"] != cb["kernel_launches"]
            finally:
                h.close()
    finally:
        d.close(); s.close()


def test_network_equals_the_oracle_directly(table_a):
    orc = O.Oracle("fz_nz", data=table_a["dense"].astype(np.float64))
    s = fw.Engine("fz_nz", table_a["n"], table_a["p"], max_k=3)
    try:
        s.set_data(table_a["triple"], csc_resident=True)
        got = s.lgl(feed_forward=True, round_size=1)
        exp = orc.learn(max_k=3, feed_forward=True, round_size=1)
        assert set(got["edges"]) == set(exp["edges"]) and len(exp["edges"]) > 0
        for e, w in exp["edges"].items():
            assert got["edges"][e] == w  # (the tolerance tests/test_gpu_fznz.py applies against the oracle: none)
        assert s.counters()["cond_tests_ref"] == exp["n_cond_tests"]
    finally:
        s.close()
        orc.close()


def test_sequential_branch_identical(table_b):
    d, s = _engines(table_b, max_k=3)
    try:
        T, Cn, A = _jobs(table_b["p"], (0, 7), (0, 1, 3, 5), 9)
        a, b = d.test_subsets_batch(T, Cn, A), s.test_subsets_batch(T, Cn, A)
        assert _subsets_bytes(a) == _subsets_bytes(b)
        assert sum(r["num_tests"] > 0 for r in a) > 10
        kw = dict(feed_forward=True, round_size=1, track_rejections=True, edge_dict=False)
        na, nb = d.lgl(**kw), s.lgl(**kw)
        assert _net_bytes(na) == _net_bytes(nb)
        assert d.counters()["cond_tests_ref"] > 0 and len(na["edge_src"]) > 0
    finally:
        d.close(); s.close()


def test_goldens_with_csc_resident():
    # as tests/test_gpu_sparse.py::test_goldens_from_sparse_input, the device keeping the table sparse as well
    raw, header, _ = fio.read_table(GOLDEN + "/HMP_SRA_gut_small.tsv")
    for max_k in (0, 3):
        net = fw.learn_network(sp.csc_matrix(raw), sensitive=True, heterogeneous=True, max_k=max_k, track_rejections=True, csc_resident=True)
        exp = read_edgelist("%s/learning_expected/exp_fz_nz_maxk%d.edgelist" % (GOLDEN, max_k))
        assert set(net["edges"]) == set(exp), max_k
        assert all(abs(net["edges"][e] - exp[e]) <= 2e-5 for e in exp), max_k
        ref = fw.learn_network(sp.csc_matrix(raw), sensitive=True, heterogeneous=True, max_k=max_k, track_rejections=True)
        assert net["edges"] == ref["edges"] and net["rejections"] == ref["rejections"]
        assert net["counters"]["csc_resident"] is True and ref["counters"]["csc_resident"] is False
        assert net["parameters"]["csc_resident"] is True and ref["parameters"]["csc_resident"] is False
        assert 0 < net["counters"]["data_resident_bytes"] < ref["counters"]["data_resident_bytes"]


def test_prepared_matrix_with_csc_resident():
    # normalize=False: a prepared Float32 CSC matrix goes up as it is
    raw, header, _ = fio.read_table(GOLDEN + "/HMP_SRA_gut_small.tsv")
    mat, _, _ = fw.normalize_counts(sp.csc_matrix(raw), "fz_nz")
    kw = dict(sensitive=True, heterogeneous=True, max_k=3, normalize=False, track_rejections=True)
    a, b = fw.learn_network(mat, **kw), fw.learn_network(mat, csc_resident=True, **kw)
    assert a["edges"] == b["edges"] and a["rejections"] == b["rejections"] and len(a["edges"]) > 0
    n, p = mat.shape
    W = (n + 63) // 64
    assert b["counters"]["data_resident_bytes"] == 12 * p * W + 4 * int(np.count_nonzero(mat.data))
    assert a["counters"]["data_resident_bytes"] == 4 * n * p + 8 * p * W


def test_resident_bytes(table_a):
    big = np.asfortranarray(_factor_table(2000, 300, 0.03, 4, 0.5))
    for t in (table_a, dict(n=2000, p=300, dense=big, triple=_triple(big), nnz=int(np.count_nonzero(big)))):
        d, s = _engines(t, max_k=0)
        try:
            n, p, W = t["n"], t["p"], (t["n"] + 63) // 64
            assert s.data_resident_bytes() == 12 * p * W + 4 * t["nnz"]
            assert d.data_resident_bytes() == 4 * n * p + 8 * p * W
        finally:
            d.close(); s.close()
    e = fw.Engine("fz_nz", 10, 3, max_k=0)
    try:
        with pytest.raises(fw.FlashWeaveError) as ei:
            e.data_resident_bytes()  # nothing uploaded yet
        assert ei.value.code == -3
    finally:
        e.close()


def test_device_never_holds_the_dense_matrix():
    """40 000 x 3 000 at 1 % fill in a fresh process: 4 n p = 480 MB, far above any allocator granularity, against 34.5 MB of plane and
    base and under 5 MB of values.  Between "before the upload" and the lowest point seen after the upload, after level 0 and after
    the network, the device's free memory may drop by less than half of 4 n p = 240 MB.  The bound follows from the sizes, not from
    a measurement.  The dense-resident upload of the same table, measured the same way, must show more than that half: the
    measurement sees a matrix of this size when there is one."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "cscres_mem_worker.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print("cscres_mem_worker:", r)
    n, p, W = r["n"], r["p"], (r["n"] + 63) // 64
    assert r["dense_matrix_bytes"] == 480_000_000 and 1_000_000 < r["nnz"] < 1_400_000
    assert r["csc_resident_bytes"] == 12 * p * W + 4 * r["nnz"] and r["dense_resident_bytes"] == 4 * n * p + 8 * p * W
    assert r["csc_drop_bytes"] < r["dense_matrix_bytes"] // 2, r
    assert r["dense_drop_bytes"] > r["dense_matrix_bytes"] // 2, r
    assert r["csc_edges"] == r["dense_edges"]


def test_reupload_in_the_other_layout(table_a):
    n, p, W = table_a["n"], table_a["p"], (table_a["n"] + 63) // 64
    eng = fw.Engine("fz_nz", n, p, max_k=3)
    try:
        kw = dict(feed_forward=True, round_size=1, edge_dict=False)
        nets = []
        for layout in ("csc", "dense", "csc", "triple", "csc"):
            if layout == "csc":
                eng.set_data(table_a["triple"], csc_resident=True)
                assert eng.data_resident_bytes() == 12 * p * W + 4 * table_a["nnz"]
            else:
                eng.set_data(table_a["dense"] if layout == "dense" else table_a["triple"])
                assert eng.data_resident_bytes() == 4 * n * p + 8 * p * W
            nets.append(_net_bytes(eng.lgl(**kw)))
        assert all(x == nets[0] for x in nets[1:])
    finally:
        eng.close()


def _bad_triples(cp, rv, n):
    """The broken triples of tests/test_gpu_sparse.py (structure only: an fz_nz upload takes any value)."""
    j = int(np.argmax(np.diff(cp) >= 3))
    a = int(cp[j])

    def mod(f):
        c2, r2 = cp.copy(), rv.copy()
        f(c2, r2)
        return c2, r2

    def swap(c, r):
        r[a], r[a + 1] = r[a + 1], r[a]

    def dup(c, r):
        r[a + 1] = r[a]

    def high(c, r):
        r[int(c[j + 1]) - 1] = n

    def colptr(c, r):
        c[j + 1] = c[j] - 1

    return j, [("unsorted", mod(swap)), ("duplicate", mod(dup)), ("row = n", mod(high)), ("colptr", mod(colptr))]


def test_bad_triples_are_refused_with_the_same_words_and_leave_the_context_as_it_was(table_a):
    cp, rv, v = table_a["triple"]
    j, bad = _bad_triples(cp, rv, table_a["n"])
    eng = fw.Engine("fz_nz", table_a["n"], table_a["p"], max_k=0)
    other = fw.Engine("fz_nz", table_a["n"], table_a["p"], max_k=0)
    try:
        eng.set_data(table_a["triple"], csc_resident=True)
        exp = eng.pw_univar_neighbors()
        for tag, (c2, r2) in bad:
            with pytest.raises(fw.FlashWeaveError) as ei:
                eng.set_data((c2, r2, v), csc_resident=True)
            with pytest.raises(fw.FlashWeaveError) as eo:
                other.set_data((c2, r2, v))
            assert ei.value.code == eo.value.code == -1 and "column %d" % j in str(ei.value), tag
            # the same words after the name of the entry point
            assert str(ei.value).split("fw_set_data_csc_f32_resident: ", 1)[1] == str(eo.value).split("fw_set_data_csc_f32: ", 1)[1], tag
            assert eng.data_resident_bytes() == 12 * table_a["p"] * 3 + 4 * table_a["nnz"]
            got = eng.pw_univar_neighbors()  # the context still holds the good upload and still works
            for k in ("off", "idx", "stat", "pval"):
                assert got[k].tobytes() == exp[k].tobytes(), (tag, k)
        P = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        for args in ((None, rv, v), (cp, None, v), (cp, rv, None)):
            assert eng.L.fw_set_data_csc_f32_resident(eng.h, *[P(a) for a in args]) == -1 and b"NULL array" in eng.L.fw_last_error(eng.h)
        # no stored entry at all: every cell an absence, level 0 finds nothing and nothing faults
        assert eng.L.fw_set_data_csc_f32_resident(eng.h, P(np.zeros(table_a["p"] + 1, np.int64)), None, None) == 0
        assert eng.level0() == 0 and eng.data_resident_bytes() == 12 * table_a["p"] * 3 + 4
    finally:
        eng.close()
        other.close()


def test_refused_on_other_kinds_and_without_recursive_pcor(table_a):
    cp, rv, v = np.array([0, 1, 1, 2], np.int64), np.array([0, 4], np.int32), np.array([1.5, 2.5], np.float32)
    eng = fw.Engine("mi_nz", 10, 3, max_k=0)
    try:
        rc = eng.L.fw_set_data_csc_f32_resident(eng.h, cp.ctypes.data_as(C.c_void_p), rv.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
        assert rc == -1 and b"FW_FZ_NZ" in eng.L.fw_last_error(eng.h)  # FW_ERR_ARG
    finally:
        eng.close()
    eng = fw.Engine("fz_nz", table_a["n"], table_a["p"], max_k=3, recursive_pcor=False)
    try:
        with pytest.raises(fw.FlashWeaveError) as ei:
            eng.set_data(table_a["triple"], csc_resident=True)
        assert ei.value.code == -5 and "recursive_pcor" in str(ei.value)  # FW_ERR_LIMIT
        eng.set_data(table_a["triple"])  # the dense-resident layout serves it
        assert eng.level0() > 0
    finally:
        eng.close()
