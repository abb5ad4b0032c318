"""Sparse (CSC) count tables end to end: fw_normalize_counts_csc, fw_set_data_csc_f32 and learn_network(scipy.sparse).
The yardstick is the dense path, which other files pin to the oracle and to the reference's goldens: sparse in == dense in,
byte for byte -- no floating-point tolerance anywhere except where a golden edge list (printed digits) is the expectation."""
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
from flashweave_jl_amd import synth
from tests.util import GOLDEN, ROOT, read_edgelist

pytestmark = pytest.mark.gpu

KINDS = ["fz", "fz_nz", "mi", "mi_nz"]
NET_KEYS = ("pc_off", "pc_idx", "pc_weight", "pc_pval", "edge_src", "edge_dst", "edge_weight")


def _golden():
    raw, header, _ = fio.read_table(GOLDEN + "/HMP_SRA_gut_small.tsv")
    return raw, header


def _random_counts(n, p, fill, seed):
    m = sp.random(n, p, density=fill, format="csc", random_state=np.random.default_rng(seed),
                  data_rvs=lambda k: 1 + np.floor(np.exp(np.random.default_rng(seed + 1).normal(1.0, 1.5, k))))
    return np.asarray(m.toarray(), dtype=np.int64)


def _special_columns():
    """An all-zero column, a constant non-zero column without zeros, a column without a single zero that varies (5 % fill elsewhere)."""
    X = _random_counts(300, 101, 0.05, 40)
    X[:, 0] = 0
    X[:, 1] = 7
    X[:, 2] = 1 + (np.arange(300) % 5)
    return X


def _special_samples():
    """Samples without reads (rows 3, 4) and a sample with exactly one read (row 5, a count of 1 in column 10); the constant
    column 1 gives every row a count, and is dropped before the samples are looked at."""
    X = _random_counts(300, 101, 0.05, 41)
    X[:, 0] = 0
    X[[3, 4, 5], :] = 0
    X[5, 10] = 1
    X[:, 1] = 7
    return X


def _tables():
    yield "hmp", _golden()[0]
    yield "fill0.5%", _random_counts(600, 333, 0.005, 10)   # 333 kept-or-not columns: never a multiple of the 64 column chunks
    yield "fill5%", _random_counts(600, 333, 0.05, 20)
    yield "fill60%", _random_counts(257, 131, 0.60, 30)
    yield "special-columns", _special_columns()
    yield "special-samples", _special_samples()
    yield "synthHE", synth.generate(400, 257, 6, mode="F", habitats=4)
    big = _random_counts(40000, 7, 0.02, 50)                # one column with 20 000 non-zeros: the device-memory sort path
    big[::2, 3] = 1 + (np.arange(20000) % 977)
    yield "long-column", big


# tables a kind may refuse in both forms (same code, same words).  Every other (table, kind) must be normalised and compared.
MAY_BE_REFUSED = {}


def _norm(x, kind):
    try:
        return fw.normalize_counts(x, kind), None
    except fw.FlashWeaveError as e:
        return None, (e.code, str(e).split(": ", 1)[1])


@pytest.mark.parametrize("kind", KINDS)
def test_frontend_sparse_equals_dense(kind):
    for tag, X in _tables():
        dense, derr = _norm(X, kind)
        sparse, serr = _norm(sp.csc_matrix(X), kind)
        assert derr == serr, (tag, derr, serr)  # a table one form refuses, the other refuses with the same words
        if derr is not None:
            assert tag in MAY_BE_REFUSED.get(kind, ()), (tag, kind, derr)  # the named cases are compared, never waved through
            continue
        (d, drm, dcm), (s, srm, scm) = dense, sparse
        if tag == "long-column" and kind == "mi_nz":
            assert dcm[3]  # the 20 000-entry column is kept: its sort ran through device memory (M > 16 384) in both forms
        assert np.array_equal(drm, srm) and np.array_equal(dcm, scm), tag
        if kind == "fz":
            assert isinstance(s, np.ndarray)
        else:
            assert sp.issparse(s) and s.format == "csc" and s.dtype == d.dtype, tag
            assert s.has_sorted_indices and np.all(np.diff(s.indptr) >= 0)
            if kind != "fz_nz":
                assert np.all(s.data != 0), tag
            s = s.toarray()
        assert s.shape == d.shape and s.dtype == d.dtype, (tag, s.shape, d.shape)
        assert np.ascontiguousarray(s).tobytes() == np.ascontiguousarray(d).tobytes(), (tag, kind, int((s != d).sum()))
    assert tag == "long-column"


def test_frontend_special_table_is_what_it_claims():
    # the special cases are really hit: dropped columns / samples, a stored 0.0f for the one-read sample, a long column
    out, rm, cm = fw.normalize_counts(sp.csc_matrix(_special_columns()), "fz_nz")
    assert not cm[0] and not cm[1] and cm[2] and rm.all()
    X = _special_samples()
    out, rm, cm = fw.normalize_counts(sp.csc_matrix(X), "fz_nz")
    assert not cm[0] and not cm[1] and cm[10] and not rm[3] and not rm[4] and rm[5]
    r5 = int(rm[:5].sum())
    row = out.tocsr()[r5]
    assert row.nnz == 1 and row.data[0] == 0.0  # log(1 / geometric mean 1): present, value exactly 0
    big = dict(_tables())["long-column"]
    assert (big[:, 3] != 0).sum() > 16384


def _net_bytes(net):
    return {k: net[k].tobytes() for k in NET_KEYS}


def test_upload_csc_f32_equals_dense_upload():
    X = synth.generate(150, 300, 9, mode="S", habitats=4)
    X[0, :] = 0
    X[0, int(np.argmax((X != 0).sum(0)))] = 1  # a sample with one read: its clr_nz value is exactly 0.0f
    mat, _, _ = fw.normalize_counts(sp.csc_matrix(X), "fz_nz")
    assert np.any(mat.data == 0.0)  # stored zeros travel through the triple form as they are
    n, p = mat.shape
    outs = []
    for form in ("dense", "triple", "scipy"):
        eng = fw.Engine("fz_nz", n, p, max_k=3)
        try:
            eng.set_data(mat.toarray() if form == "dense" else (mat.indptr, mat.indices, mat.data) if form == "triple" else mat)
            nb = eng.pw_univar_neighbors()
            net = eng.lgl(feed_forward=True, round_size=1, track_rejections=True)
            outs.append((nb, net))
        finally:
            eng.close()
    (nb0, net0) = outs[0]
    assert len(nb0["idx"]) > 0
    for nb, net in outs[1:]:
        for k in ("off", "idx", "stat", "pval"):
            assert nb[k].tobytes() == nb0[k].tobytes(), k
        assert _net_bytes(net) == _net_bytes(net0)
        assert net["rejection_records"].tobytes() == net0["rejection_records"].tobytes()


def test_upload_csc_f32_refused_on_other_kinds():
    eng = fw.Engine("mi_nz", 10, 3, max_k=0)
    try:
        cp, rv, v = np.array([0, 1, 1, 2], np.int64), np.array([0, 4], np.int32), np.array([1.5, 2.5], np.float32)
        rc = eng.L.fw_set_data_csc_f32(eng.h, cp.ctypes.data_as(C.c_void_p), rv.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p))
        assert rc == -1 and b"FW_FZ_NZ" in eng.L.fw_last_error(eng.h)
    finally:
        eng.close()


def test_upload_csc_f32_null_arrays():
    eng = fw.Engine("fz_nz", 100, 3, max_k=0)
    try:
        cp, rv, v = np.array([0, 1, 1, 2], np.int64), np.array([0, 40], np.int32), np.array([1.5, 2.5], np.float32)
        P = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        for args in ((None, rv, v), (cp, None, v), (cp, rv, None)):
            assert eng.L.fw_set_data_csc_f32(eng.h, *[P(a) for a in args]) == -1  # FW_ERR_ARG
            assert b"NULL array" in eng.L.fw_last_error(eng.h)
        empty = np.zeros(4, np.int64)  # no stored entry: the two arrays may be NULL, every cell is an absence
        assert eng.L.fw_set_data_csc_f32(eng.h, P(empty), None, None) == 0
        eng.set_data((cp, rv, v))
        assert eng.level0() >= 0
    finally:
        eng.close()


def _same_result(a, b, tag):
    assert a["variable_ids"] == b["variable_ids"], tag
    assert set(a["edges"]) == set(b["edges"]), tag
    assert all(a["edges"][e] == b["edges"][e] for e in a["edges"]), tag
    assert a["rejections"] == b["rejections"], tag


@pytest.mark.parametrize("sensitive", [True, False])
@pytest.mark.parametrize("heterogeneous", [True, False])
def test_learn_network_sparse_equals_dense(sensitive, heterogeneous):
    raw, header = _golden()
    synthetic = synth.generate(800, 400, 7, mode="S" if sensitive else "F", habitats=4 if heterogeneous else 0)
    for tag, X, hdr in (("hmp", raw, header), ("synthetic", synthetic, None)):
        for max_k in (0, 3):
            kw = dict(sensitive=sensitive, heterogeneous=heterogeneous, max_k=max_k, header=hdr, track_rejections=True)
            d = fw.learn_network(X, **kw)
            s = fw.learn_network(sp.csc_matrix(X), **kw)
            _same_result(d, s, (tag, max_k))
            assert s["counters"]["sparse_input"] is True and s["counters"]["normalized_on_device"] is True
            assert d["counters"]["sparse_input"] is False
            if tag == "synthetic":
                assert len(d["variable_ids"]) > 512  # device rounds
            if max_k == 3 and tag == "synthetic":
                assert len(d["edges"]) > 0


@pytest.mark.parametrize("name", ["mi_nz", "fz_nz"])
def test_learn_network_prepared_sparse_matrix(name):
    X = synth.generate(800, 400, 8, mode="F" if name == "mi_nz" else "S", habitats=4)
    mat, _, _ = fw.normalize_counts(X, name)
    kw = dict(sensitive=name == "fz_nz", heterogeneous=True, max_k=3, normalize=False, track_rejections=True)
    d = fw.learn_network(mat, **kw)
    s = fw.learn_network(sp.csc_matrix(mat), **kw)
    _same_result(d, s, name)
    assert len(d["edges"]) > 0 and s["counters"]["sparse_input"] is True and s["counters"]["normalized_on_device"] is False


def test_goldens_from_sparse_input():
    # as test_gpu_rejections.py::test_learn_network_golden_table_with_track_rejections, the counts wrapped in a csc_matrix
    raw, header, _ = fio.read_table(GOLDEN + "/HMP_SRA_gut_small.tsv")
    for sensitive, name, wtol in ((True, "fz_nz", 2e-5), (False, "mi_nz", 1e-13)):
        for max_k in (0, 3):
            net = fw.learn_network(sp.csc_matrix(raw), sensitive=sensitive, heterogeneous=True, max_k=max_k, track_rejections=True)
            exp = read_edgelist("%s/learning_expected/exp_%s_maxk%d.edgelist" % (GOLDEN, name, max_k))
            assert set(net["edges"]) == set(exp), (name, max_k)
            assert all(abs(net["edges"][e] - exp[e]) <= wtol for e in exp), (name, max_k)


def test_host_never_densifies():
    """60 000 x 8 000 at 0.5 % fill, built in CSC form (2.4 M entries, ~30 MB), mi_nz at max_k = 0 in a fresh process: the peak
    resident set may grow by less than 0.96 GB = half of ONE dense Int32 copy (1.92 GB) between "library loaded" and "network
    returned".  The bound follows from the size, not from a measurement; the dense path holds at least two such copies.
    ru_maxrss is a high-water mark that importing the libraries can already have pushed above what the process holds afterwards
    (then its growth alone would show nothing), so the resident set sampled every 2 ms during the call is held to the same bound;
    its baseline is taken after a small table has been learnt in the same process, so that what the first device call maps
    whatever the size of the table (HIP runtime, code objects) is not counted as the table's."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sparse_rss_worker.py")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print("sparse_rss_worker:", r)
    assert r["sparse_input"] and r["normalized_on_device"]
    assert r["dense_int32_bytes"] == 1_920_000_000 and 2_000_000 < r["nnz"] < 2_800_000
    assert r["variables"] > 1000
    assert r["growth_bytes"] < 0.96e9, r
    assert r["n_samples"] > 10 and r["sampled_growth_bytes"] < 0.96e9, r


def _bad_triples():
    X = _random_counts(50, 9, 0.3, 60)
    m = sp.csc_matrix(X.astype(np.int32))
    m.sort_indices()
    cp, rv, v = m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.int32)
    j = int(np.argmax(np.diff(cp) >= 3))
    a = int(cp[j])

    def mod(f):
        c2, r2, v2 = cp.copy(), rv.copy(), v.copy()
        f(c2, r2, v2)
        return j, (c2, r2, v2, X.shape)

    def swap(c, r, x):
        r[a], r[a + 1] = r[a + 1], r[a]

    def dup(c, r, x):
        r[a + 1] = r[a]

    def high(c, r, x):
        r[int(c[j + 1]) - 1] = X.shape[0]

    def zero(c, r, x):
        x[a + 1] = 0

    def neg(c, r, x):
        x[a + 2] = -4

    def colptr(c, r, x):
        c[j + 1] = c[j] - 1

    return X, [("unsorted", mod(swap)), ("duplicate", mod(dup)), ("row = n", mod(high)), ("stored zero", mod(zero)),
               ("negative", mod(neg)), ("colptr", mod(colptr))]


def _raw_normalize(triple, kind):
    """fw_normalize_counts_csc on a triple exactly as given (normalize_counts would canonicalise it first)."""
    L = fw.load_library()
    cp, rv, v, (n, p) = triple
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    nnz = max(int(cp[-1]), len(rv), 1)
    ocp, orow, oi, of = np.zeros(p + 1, np.int64), np.zeros(nnz, np.int32), np.zeros(nnz, np.int32), np.zeros(max(nnz, n * p), np.float32)
    rm, cm = np.zeros(n, np.uint8), np.zeros(p, np.uint8)
    no, po, nz = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    rc = L.fw_normalize_counts_csc(0, fw.engine._KINDS[kind], n, p, P(cp), P(rv), P(v), P(ocp), P(orow), P(oi), P(of), P(rm), P(cm),
                                   C.byref(no), C.byref(po), C.byref(nz))
    return rc, L.fw_last_error(None).decode()


def test_validation_on_the_device_and_no_state_leaks():
    X, bad = _bad_triples()
    good, grm, gcm = fw.normalize_counts(X, "mi_nz")
    for tag, (j, triple) in bad:
        rc, msg = _raw_normalize(triple, "mi_nz")
        assert rc == -1, (tag, rc, msg)  # FW_ERR_ARG
        assert "column %d" % j in msg, (tag, msg)
        out, rm, cm = fw.normalize_counts(sp.csc_matrix(X), "mi_nz")  # the same process, right afterwards
        assert np.array_equal(out.toarray(), good) and np.array_equal(rm, grm) and np.array_equal(cm, gcm), tag
    # the sparse fz_nz upload checks the structure the same way (values may be anything there) and recovers the same way
    mat, _, _ = fw.normalize_counts(sp.csc_matrix(X), "fz_nz")
    n, p = mat.shape
    m2 = mat.copy()
    m2.sort_indices()
    cp, rv, v = m2.indptr.astype(np.int64), m2.indices.astype(np.int32), m2.data.astype(np.float32)
    j = int(np.argmax(np.diff(cp) >= 2))
    eng = fw.Engine("fz_nz", n, p, max_k=0)
    ref = fw.Engine("fz_nz", n, p, max_k=0)
    try:
        ref.set_data(mat.toarray())
        exp = ref.pw_univar_neighbors()
        for tag in ("unsorted", "row = n", "colptr"):
            c2, r2 = cp.copy(), rv.copy()
            if tag == "unsorted":
                r2[cp[j]], r2[cp[j] + 1] = r2[cp[j] + 1], r2[cp[j]]
            elif tag == "row = n":
                r2[cp[j + 1] - 1] = n
            else:
                c2[j + 1] = c2[j] - 1
            with pytest.raises(fw.FlashWeaveError) as ei:
                eng.set_data((c2, r2, v))
            assert ei.value.code == -1 and "column %d" % j in str(ei.value), tag
            with pytest.raises(fw.FlashWeaveError) as ei:
                eng.level0()  # a refused upload leaves no data behind
            assert ei.value.code == -3
            eng.set_data((cp, rv, v))
            got = eng.pw_univar_neighbors()
            for k in ("off", "idx", "stat", "pval"):
                assert got[k].tobytes() == exp[k].tobytes(), (tag, k)
    finally:
        eng.close()
        ref.close()
