"""Real-valued tables on the device: fw_normalize_abund / fw_normalize_abund_csc (the Float64 instantiation of csrc/fw_norm.hip),
engine.normalize_abundances and learn_network(abundances=True).
Yardsticks: the count path for tables of integers (byte for byte: the two instantiations share every expression), the host front-end
(preprocess.py) for real values, the dense form for the CSC form (byte for byte).
The host yardstick is called with tie_anchor=True: the anchor rule abundances=True asks for on either front-end (the first sample
whose sum lies within width * 2^-52 of the largest; preprocess.adaptive_clr).  The plain rule (the largest Float64 sum, the default
of the host front-end and the reference's findmax) is decided by the order of the additions in a table whose samples all sum to 1,
so no front-end with another order can be held to it.  Every fz comparison first asserts on the host that the table's anchor is
unique under the tolerant rule (_assert_anchor_is_separated): no sum lies in the margin around the window's edge.
Tolerance of the continuous kinds against the host: the one tests/test_gpu_norm.py derives -- both compute in Float64 and return
Float32, the device's log and numpy's can differ in the last Float64 bit, which survives the rounding to Float32 in rare cases:
one Float32 ulp (rtol 2.4e-7), nearly every entry the same Float32.  The derivation does not involve the value type.
The discrete kinds are exact.  For mi_nz that needs a precondition on the table, which every mi_nz comparison asserts on the host
first (_assert_no_near_ties): two clr keys of one column lie more than 1e-9 apart -- six orders of magnitude above Float64
rounding -- or belong to rows that are exact duplicates, so no tied rank can hang on a summation order."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import io as fio
from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd import synth
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

KINDS = ["fz", "fz_nz", "mi", "mi_nz"]
MODES = {"fz": dict(sensitive=True, heterogeneous=False), "fz_nz": dict(sensitive=True, heterogeneous=True),
         "mi": dict(sensitive=False, heterogeneous=False), "mi_nz": dict(sensitive=False, heterogeneous=True)}


def _rows_to_one(x, scale=1.0):
    """every sample with reads divided by its sum (times scale); samples without reads stay zero"""
    x = np.asarray(x, dtype=np.float64)
    s = x.sum(axis=1, keepdims=True)
    return x / np.where(s > 0, s, 1.0) * scale


def _dup_counts():
    """the table of tests/test_gpu_norm.py::test_binned_nz_clr_ties_and_duplicated_samples: 50 duplicated samples"""
    rng = np.random.default_rng(3)
    base = rng.poisson(3.0, size=(150, 60)) * (rng.random((150, 60)) < 0.6)
    return np.concatenate([base, base[:50]], axis=0)


def _random_real(n, p, fill, seed):
    m = sp.random(n, p, density=fill, format="csc", random_state=np.random.default_rng(seed),
                  data_rvs=lambda k: np.exp(np.random.default_rng(seed + 1).normal(-3.0, 1.5, k)))
    return np.asarray(m.toarray(), dtype=np.float64)


@functools.lru_cache(maxsize=None)
def _table(tag):
    if tag == "hmp_counts":
        return np.asarray(fio.read_table(GOLDEN + "/HMP_SRA_gut_small.tsv")[0]).astype(np.int64)
    if tag == "synth_counts":
        return synth.generate(300, 211, 5)
    if tag == "dup_counts":
        return _dup_counts()
    if tag == "relS":  # relative abundances, fill 0.58, smallest value 3.3e-5: the floor of clr_adapt is a tenth of it
        x = synth.generate(300, 211, 5, mode="S").astype(np.float64)
        x[:, 17] = 0
        x[40, :] = 0
        return _rows_to_one(x)
    if tag == "pctF":  # percentages: values on both sides of 1, and a constant dyadic column
        x = _rows_to_one(synth.generate(200, 257, 6, mode="F", habitats=4), 100.0)
        x[:, 9] = 0.25
        return x
    if tag == "dup":
        return _rows_to_one(_dup_counts())
    if tag == "dup1.5":  # non-integral, smallest value >= 1: the base = 1 branch
        return 1.5 * _dup_counts()
    if tag == "hmp":
        return _rows_to_one(_table("hmp_counts"))
    if tag.startswith("fill"):
        fill, seed = {"fill0.5%": (0.005, 10), "fill5%": (0.05, 20), "fill60%": (0.60, 30)}[tag]
        return _random_real(130, 70, fill, seed)  # n no multiple of 64, kept columns few next to the 64 chunks
    if tag == "few-columns":  # fewer than 64 kept columns; column 3 with a single entry; sample 7 holds its one OTU alone
        x = _random_real(90, 40, 0.30, 60)
        x[:, 3] = 0
        x[11, 3] = 0.125
        x[7, :] = 0
        x[7, 5] = 0.0625
        return x
    if tag == "long-column":  # one CSC column of more than 2 048 stored entries: csc_binned_kernel's 1 024-thread form
        rng = np.random.default_rng(70)
        x = np.exp(rng.normal(-3.0, 1.5, (2100, 8))) * (rng.random((2100, 8)) < 0.05)
        x[:, 0] = np.exp(rng.normal(-3.0, 1.5, 2100))
        x[:, 1] = np.exp(rng.normal(-3.0, 1.5, 2100)) * (np.arange(2100) % 41 != 0)
        x[::41, 2] = np.exp(rng.normal(-3.0, 1.5, 52))  # (two values in every sample: a sample of one value has the key ~0)
        return x
    if tag == "beyond-lds":  # 16 500 kept samples, distinct real values, no duplicated rows: the sort keys leave LDS
        rng = np.random.default_rng(74)  # (a draw whose 16 500 keys per column keep the 1e-9 gap the test asserts; most do)
        x = np.exp(rng.normal(-3.0, 1.5, (16500, 6))) * (rng.random((16500, 6)) < 0.5)
        x[:, :2] = np.exp(rng.normal(-3.0, 1.5, (16500, 2)))  # (two values in every sample: a sample of one value has the key ~0)
        return x
    raise KeyError(tag)


@functools.lru_cache(maxsize=None)
def _host(tag, kind):
    """the host front-end's answer, computed once per (table, kind) and shared"""
    out = pre.normalize(_table(tag), kind, prec=32, tie_anchor=True)
    for a in out:
        a.setflags(write=False)
    return out


def _power_of_two_row(row):
    """every non-zero of the sample is one value 2^k, and the host's clr_nz keys of the sample are exactly 0.0"""
    v = np.unique(row[row != 0])
    return v.size == 1 and np.frexp(v[0])[0] == 0.5 and not pre.clr_nz(row[None, :]).any()


def _assert_anchor_is_separated(tag):
    """The precondition of an fz comparison: the anchor of clr_adapt is unique under the tolerant rule.  With d = (largest sum - sum) /
    largest sum of the filtered table and w = width * 2^-52, every sample has d <= w / 4 (inside the window whatever the order of the
    additions: another order moves a sum by a few ulps, and w / 4 is width / 4 ulps with widths of 40 and more here) or d >= 4 w
    (outside it whatever the order); the anchor is then the first sample inside."""
    x, _, _ = pre.filter_by_variance(_table(tag))
    depth = x.sum(axis=1)
    d, w = (depth.max() - depth) / depth.max(), x.shape[1] * 2.0 ** -52
    assert np.all((d <= w / 4) | (d >= 4 * w)), (tag, np.sort(d[(d > w / 4) & (d < 4 * w)]) / w)


def _assert_no_near_ties(tag, power_of_two_rows=False):
    """The precondition of an exact mi_nz comparison: within a column, two clr_nz keys lie more than 1e-9 apart or their rows are
    exact duplicates (keys of the filtered table, computed here in one vectorised pass).
    power_of_two_rows (the HMP fixture alone, which holds two such pairs: samples of counts (1), (1, 1) become (1.0), (0.5, 0.5)): a
    pair may also tie when all non-zeros of each sample are one power of two.  Such a sample's key is log(v / exp(log v)): log(2^k) is
    k ln 2 in one rounding, its mean over equal terms is the term, and exp returns 2^k (the rounding error of ln 2, 2.3e-17 relative,
    is a fifth of half an ulp), so the key is exactly 0.0 on either side.  For any other value v the same key is 0 or one ulp off
    by the grace of two libms: the generated tables avoid samples of one value."""
    x, _, _ = pre.filter_by_variance(_table(tag))
    present = x != 0
    logs = np.where(present, np.log(np.where(present, x, 1.0)), 0.0)
    keys = logs - (logs.sum(axis=1) / np.maximum(present.sum(axis=1), 1))[:, None]
    for j in range(x.shape[1]):
        rows = np.nonzero(present[:, j])[0]
        order = rows[np.argsort(keys[rows, j], kind="stable")]
        close = np.nonzero(np.diff(keys[order, j]) <= 1e-9)[0]
        for k in close:
            a, b = x[order[k]], x[order[k + 1]]
            assert np.array_equal(a, b) or (power_of_two_rows and _power_of_two_row(a) and _power_of_two_row(b)), \
                (tag, j, int(order[k]), int(order[k + 1]))


def _bytes(out):
    """a front-end's output as (type, shape, raw bytes of the dense form, stored-entry count)"""
    if sp.issparse(out):
        assert out.format == "csc" and out.has_sorted_indices
        return out.dtype, out.shape, np.ascontiguousarray(out.toarray()).tobytes(), int(out.nnz)
    return out.dtype, out.shape, np.ascontiguousarray(out).tobytes(), None


def _norm(front_end, x, kind):
    try:
        return front_end(x, kind), None
    except fw.FlashWeaveError as e:
        return None, (e.code, str(e).split(": ", 1)[1])


# 1 ---- the Float64 instantiation on tables of integers is the count path, byte for byte ---------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_integer_tables_equal_the_count_path(kind):
    for tag in ("hmp_counts", "synth_counts", "dup_counts"):
        counts = _table(tag)
        for form in (np.asarray, sp.csc_matrix):
            exp, erm, ecm = fw.normalize_counts(form(counts), kind)
            got, rm, cm = fw.normalize_abundances(form(counts.astype(np.float64)), kind)
            assert np.array_equal(rm, erm) and np.array_equal(cm, ecm), (tag, form.__name__)
            assert _bytes(got) == _bytes(exp), (tag, form.__name__)
            if sp.issparse(exp):
                assert np.array_equal(got.indptr, exp.indptr) and np.array_equal(got.indices, exp.indices)
                assert got.data.tobytes() == exp.data.tobytes()


# 2 ---- real-valued tables against the host front-end ------------------------------------------------------------------------------
def _check_against_host(tag, kind, got, rm, cm):
    exp, erm, ecm = _host(tag, kind)
    assert np.array_equal(rm, erm) and np.array_equal(cm, ecm), tag
    got = got.toarray() if sp.issparse(got) else got
    assert got.shape == exp.shape, (tag, got.shape, exp.shape)
    if kind in ("mi", "mi_nz"):
        assert np.array_equal(got, exp), (tag, int((got != exp).sum()))
        if kind == "mi_nz":
            assert set(np.unique(got)) == {0, 1, 2}, tag
    else:
        print(tag, kind, "max |got - exp| = %.3g, equal share = %.6f" % (np.abs(got - exp).max(), (got == exp).mean()))
        assert np.allclose(got, exp, rtol=2.4e-7, atol=1e-7), (tag, np.abs(got - exp).max())
        assert (got == exp).mean() > 0.999, tag


@pytest.mark.parametrize("kind", KINDS)
def test_real_tables_equal_the_host_front_end(kind):
    for tag in ("relS", "pctF", "dup", "dup1.5", "hmp"):
        if kind == "mi_nz":
            _assert_no_near_ties(tag, power_of_two_rows=tag == "hmp")
        if kind == "fz":
            _assert_anchor_is_separated(tag)
        _check_against_host(tag, kind, *fw.normalize_abundances(_table(tag), kind))


def test_real_tables_are_what_they_claim():
    x = _table("relS")
    assert 0.5 < (x != 0).mean() < 0.65 and 0 < x[x > 0].min() < 1e-4  # the floor = smallest / 10 branch of clr_adapt
    assert not x[:, 17].any() and not x[40].any()
    _, rm, cm = fw.normalize_abundances(x, "fz")
    assert not cm[17] and not rm[40]
    x = _table("pctF")
    assert x[x > 0].min() < 1 < x.max()
    assert not fw.normalize_abundances(x, "fz_nz")[2][9]  # the constant 0.25 column: min == max
    assert _table("dup1.5")[_table("dup1.5") > 0].min() >= 1 and np.any(_table("dup1.5") != np.floor(_table("dup1.5")))
    with pytest.raises(TypeError):
        fw.normalize_counts(_table("dup1.5"), "fz")  # the count front-end keeps refusing what is not integral


# 3 ---- CSC equals dense for Float64 -----------------------------------------------------------------------------------------------
MAY_BE_REFUSED = {}  # tables a kind may refuse in both forms (same code, same words); every other (table, kind) is compared


@pytest.mark.parametrize("kind", KINDS)
def test_csc_equals_dense(kind):
    for tag in ("relS", "pctF", "dup", "dup1.5", "hmp", "fill0.5%", "fill5%", "fill60%", "few-columns"):
        x = _table(tag)
        dense, derr = _norm(fw.normalize_abundances, x, kind)
        sparse, serr = _norm(fw.normalize_abundances, sp.csc_matrix(x), kind)
        assert derr == serr, (tag, derr, serr)
        if derr is not None:
            assert tag in MAY_BE_REFUSED.get(kind, ()), (tag, kind, derr)
            continue
        (d, drm, dcm), (s, srm, scm) = dense, sparse
        assert np.array_equal(drm, srm) and np.array_equal(dcm, scm), tag
        if kind == "fz":
            assert isinstance(s, np.ndarray)
        else:
            assert sp.issparse(s) and s.format == "csc" and s.dtype == d.dtype, tag
            if kind != "fz_nz":
                assert np.all(s.data != 0), tag
        assert _bytes(s)[:3] == _bytes(d)[:3], (tag, kind)
        if tag == "few-columns":
            assert 0 < dcm.sum() < 64 and dcm[3] == (kind != "mi_nz") and drm[7]  # (a single entry: two levels, but one bin)
            if kind == "fz_nz":  # sample 7 holds one OTU: log(x / x) is a STORED 0.0f
                row = s.tocsr()[int(drm[:7].sum())]
                assert row.nnz == 1 and row.data[0] == 0.0


# 4 ---- the launch shapes of the binned kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["long-column", "beyond-lds"])
def test_binned_launch_shapes(tag):
    x = _table(tag)
    if tag == "long-column":
        assert x.shape[0] == 2100 and (x[:, 0] != 0).sum() > 2048 and (x[:, 1:] != 0).sum(axis=0).max() <= 2048
    else:
        assert x.shape == (16500, 6) and (x[:, 0] != 0).all() and len(np.unique(x, axis=0)) == 16500
    _assert_no_near_ties(tag)
    for form in (np.asarray, sp.csc_matrix):
        got, rm, cm = fw.normalize_abundances(form(x), "mi_nz")
        assert cm[0] and rm.sum() > (2048 if tag == "long-column" else 16384)
        _check_against_host(tag, "mi_nz", got, rm, cm)


# 5 ---- refusals on the device entry points, past the Python check -------------------------------------------------------------------
def _raw(x, sparse):
    """fw_normalize_abund / fw_normalize_abund_csc on the values exactly as given -> (rc, message)"""
    L = fw.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    n, p = x.shape
    rm, cm, no, po, nz = np.zeros(n, np.uint8), np.zeros(p, np.uint8), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    oi = np.zeros(n * p, np.int32)
    if not sparse:
        v = np.asfortranarray(x, dtype=np.float64)
        rc = L.fw_normalize_abund(0, fw.FW_MI_NZ, n, p, P(v), None, P(oi), P(rm), P(cm), C.byref(no), C.byref(po))
    else:
        present = ~(x == 0)  # (a NaN is a stored entry)
        cols, rows = np.nonzero(present.T)
        cp = np.concatenate(([0], np.cumsum(present.sum(axis=0)))).astype(np.int64)
        rv, v = rows.astype(np.int32), np.ascontiguousarray(x[rows, cols], dtype=np.float64)
        ocp, orow = np.zeros(p + 1, np.int64), np.zeros(n * p, np.int32)
        rc = L.fw_normalize_abund_csc(0, fw.FW_MI_NZ, n, p, P(cp), P(rv), P(v), P(ocp), P(orow), P(oi), None, P(rm), P(cm),
                                      C.byref(no), C.byref(po), C.byref(nz))
    return rc, L.fw_last_error(None).decode()


@pytest.mark.parametrize("sparse", [False, True])
def test_refusals_on_the_device(sparse):
    good = _table("fill60%")
    ref = fw.normalize_abundances(good, "mi_nz")[0]
    for j, bad in ((4, -0.5), (21, np.nan), (66, np.inf), (33, -np.inf)):
        x = good.copy()
        x[int(np.argmax(x[:, j] != 0)), j] = bad
        with pytest.raises(ValueError, match="normalize_abundances"):
            fw.normalize_abundances(sp.csc_matrix(x) if sparse else x, "mi_nz")  # the Python check, before any device call
        rc, msg = _raw(x, sparse)
        assert rc == -1 and "column %d" % j in msg and "fw_normalize_abund" in msg, (bad, rc, msg)  # FW_ERR_ARG
        assert np.array_equal(fw.normalize_abundances(good, "mi_nz")[0], ref)  # the same process, right afterwards
    x = good.copy()
    x[x[:, 8] == 0, 8] = -0.0  # -0.0 is a zero
    assert _bytes(fw.normalize_abundances(x, "mi_nz")[0]) == _bytes(ref)
    assert _raw(x, False)[0] == 0


# 6 ---- composition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [np.asarray, sp.csc_matrix], ids=["dense", "sparse"])
@pytest.mark.parametrize("kind", KINDS)
def test_learn_network_composes_the_front_end_and_the_engine(kind, form):
    x = form(_table("hmp"))
    d = fw.normalize_data(x, test_name=kind, abundances=True)
    exp = fw.learn_network(d["data"], normalize=False, header=d["header"], max_k=3, **MODES[kind])
    got = fw.learn_network(x, abundances=True, max_k=3, **MODES[kind])
    assert got["edges"] == exp["edges"] and got["variable_ids"] == exp["variable_ids"]
    assert len(got["edges"]) > 0 or kind == "mi_nz"  # (mi_nz finds no edge among these 346 samples: two empty networks there)
    assert got["counters"]["normalized_on_device"] is True and got["parameters"]["abundances"] is True
    assert "abundances" not in exp["parameters"]
    assert got["counters"]["sparse_input"] is sp.issparse(x)
    if kind == "fz_nz" and sp.issparse(x):
        res = fw.learn_network(x, abundances=True, max_k=3, csc_resident=True, **MODES[kind])
        assert res["edges"] == exp["edges"] and res["counters"]["csc_resident"] is True


# 7 ---- extra_data -----------------------------------------------------------------------------------------------------------------
def test_extra_data_tables_take_the_new_front_end():
    counts = _table("hmp_counts")
    half = counts.shape[1] // 2
    a, b = _rows_to_one(counts[:, :half]), _rows_to_one(counts[:, half:])
    on = fw.learn_network(a, extra_data=[(b, None)], abundances=True, max_k=1, **MODES["fz_nz"])
    assert on["counters"]["n_tables"] == 2 and on["counters"]["normalized_on_device"] is True
    off = fw.learn_network(a, extra_data=[(b, None)], max_k=1, **MODES["fz_nz"])
    assert off["counters"]["n_tables"] == 2 and off["counters"]["normalized_on_device"] is False  # today's routing: the host front-end
    assert "abundances" not in off["parameters"]
