"""learn_network(abundances=True) / normalize_data(abundances=True), the parts that need no device: which front-end a table is handed to
and in which form, the refusals (all raised before any device call), and that a call without the option is routed as before.
fw.api.Engine, fw.api.normalize_counts and fw.api.normalize_abundances are replaced by recording stand-ins, as tests/api_trace.py
does; the stand-in front-end is preprocess.normalize on the scattered table."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd.engine import CSC
from tests import api_trace
from tests.api_trace import KINDS, MASK, RecordingEngine, _scatter, counts

LOG = []  # [front-end name, the table it received, test_name]


def rel(x):
    """relative abundances of a count table (no empty sample in tests/api_trace.counts)"""
    x = np.asarray(x, dtype=np.float64)
    return x / x.sum(axis=1, keepdims=True)


def _stand_in(name):
    def front_end(table, test_name, **kw):
        LOG.append([name, table, test_name])
        if not isinstance(table, CSC):
            return pre.normalize(table, test_name)
        dense = _scatter(*table)
        data, row_mask, col_mask = pre.normalize(dense, test_name)
        if test_name == "fz":
            return data, row_mask, col_mask
        data = data.astype(np.float32 if test_name == "fz_nz" else np.int32)
        present = dense[row_mask][:, col_mask] != 0 if test_name == "fz_nz" else data != 0
        cols, rows = np.nonzero(present.T)
        out = sp.csc_matrix(data.shape, dtype=data.dtype)
        out.indptr = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=data.shape[1])))).astype(np.int32)
        out.indices, out.data = rows.astype(np.int32), data[rows, cols]
        return out, row_mask, col_mask
    return front_end


@pytest.fixture
def recorded(monkeypatch):
    del LOG[:], api_trace._LOG[:]
    monkeypatch.setattr(fw.api, "Engine", RecordingEngine)
    monkeypatch.setattr(fw.api, "normalize_counts", _stand_in("normalize_counts"))
    monkeypatch.setattr(fw.api, "normalize_abundances", _stand_in("normalize_abundances"))
    return LOG


def _is_f64_csc(t):
    m = sp.csc_matrix((t.nzval, t.rowval, t.colptr), shape=t.shape)
    return (isinstance(t, CSC) and t.nzval.dtype == np.float64 and t.colptr.dtype == np.int64 and t.rowval.dtype == np.int32 and
            m.has_canonical_format and np.all(t.nzval != 0))


def test_the_keyword_exists():
    """On the parent commit abundances falls into **unsupported (TypeError) and the function does not exist."""
    for f in (fw.learn_network, fw.normalize_data):
        assert inspect.signature(f).parameters["abundances"].default is False
    assert callable(fw.normalize_abundances) and fw.normalize_abundances is fw.engine.normalize_abundances


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_hand_off(recorded, kind, form):
    x = rel(counts())
    table = sp.coo_matrix(x) if form == "sparse" else x.astype(np.float32)  # (no canonical form, no Float64, on the way in)
    for call in (lambda: fw.learn_network(table, abundances=True, **KINDS[kind]),
                 lambda: fw.normalize_data(table, test_name=kind, abundances=True)):
        del recorded[:]
        r = call()
        assert [c[0] for c in recorded] == ["normalize_abundances"] and recorded[0][2] == kind  # and normalize_counts was not called
        got = recorded[0][1]
        if form == "sparse":
            assert _is_f64_csc(got) and np.array_equal(_scatter(*got), x)
        else:
            assert isinstance(got, np.ndarray) and got.dtype == np.float64 and np.array_equal(got, table)  # (Float32 widens exactly)
    assert sp.issparse(r["data"]) is (form == "sparse" and kind != "fz")  # (normalize_data: a sparse table stays sparse)
    r = fw.learn_network(table, abundances=True, **KINDS[kind])
    assert r["counters"]["normalized_on_device"] is True and r["counters"]["sparse_input"] is (form == "sparse")


def test_the_front_end_widens_to_float64(monkeypatch):
    seen = []

    class Lib:
        fw_normalize_abund = fw_normalize_abund_csc = None
    monkeypatch.setattr(fw.engine, "load_library", lambda: Lib)
    monkeypatch.setattr(fw.engine, "_normalize_dense", lambda fe, x, t, d: seen.append(x) or "dense")
    monkeypatch.setattr(fw.engine, "_normalize_csc", lambda fe, who, triple, t, d: seen.append(triple) or "csc")
    x32 = rel(counts()).astype(np.float32)
    for table in (x32, counts(), counts() > 4):
        assert fw.normalize_abundances(table, "fz") == "dense"
        got = seen.pop()
        assert got.dtype == np.float64 and got.flags.f_contiguous and np.array_equal(got, table)  # (Float32 widens exactly)
    assert fw.normalize_abundances(sp.csr_matrix(x32), "fz_nz") == "csc"
    assert _is_f64_csc(seen.pop())
    with pytest.raises(ValueError, match="normalize_abundances"):
        fw.normalize_abundances(rel(counts())[0], "fz")  # not two-dimensional
    for bad in (np.nan, np.inf, -np.inf, -0.25):
        x = rel(counts())
        x[2, 3] = bad
        for table in (x, sp.csc_matrix(x)):
            with pytest.raises(ValueError, match="normalize_abundances.*(NaN|negative)"):
                fw.normalize_abundances(table, "mi")
    assert not seen  # every refusal came before a device call


def test_every_extra_table_takes_the_new_front_end(recorded):
    a, b, c = rel(counts()), rel(counts(4, 2)), rel(counts(3, 5))
    r = fw.learn_network(a, extra_data=[(b, None), (c, ["b0", "b1", "b2"])], abundances=True, **KINDS["fz_nz"])
    assert [call[0] for call in recorded] == ["normalize_abundances"] * 3
    assert sorted(call[1].shape[1] for call in recorded) == [3, 4, 8]
    assert r["counters"]["n_tables"] == 3 and r["counters"]["normalized_on_device"] is True and r["parameters"]["abundances"] is True
    del recorded[:]
    d = fw.normalize_data(sp.csc_matrix(a), extra_data=[(sp.csr_matrix(b), None)], test_name="mi_nz", abundances=True)
    assert [call[0] for call in recorded] == ["normalize_abundances"] * 2 and all(_is_f64_csc(call[1]) for call in recorded)
    assert sp.issparse(d["data"])


def test_sparse_table_with_a_covariate_under_meta_mask(recorded):
    x = rel(counts())
    x[:, MASK] = np.stack([np.arange(6) % 2, 2.5 + 1.25 * (np.arange(6) % 7)], axis=1)  # a 0 / 1 column and a non-integral covariate
    d = fw.normalize_data(sp.csc_matrix(x), test_name="fz_nz", meta_mask=MASK, abundances=True)
    assert [call[0] for call in recorded] == ["normalize_abundances"]
    otu = recorded[0][1]
    assert _is_f64_csc(otu) and np.array_equal(_scatter(*otu), x[:, ~MASK])  # the OTU block alone, the covariate is no abundance
    assert sp.issparse(d["data"]) and d["data"].format == "csc"
    assert list(d["meta_mask"][-2:]) == [True, True] and not any(d["meta_mask"][:-2]) and d["header"][-2:] == ["X3", "X6"]
    r = fw.learn_network(sp.csc_matrix(x), meta_mask=MASK, abundances=True, **KINDS["fz_nz"])
    assert r["parameters"]["meta_mask"] == 2 and r["parameters"]["abundances"] is True and r["counters"]["sparse_input"] is True


def _with(value, at=(2, 3)):
    x = rel(counts(4, 2))
    x[at] = value
    return x


@pytest.mark.parametrize("form", [np.asarray, sp.csc_matrix], ids=["dense", "sparse"])
def test_refusals_come_before_any_call(recorded, form):
    good = rel(counts())
    with pytest.raises(ValueError, match="abundances=True with normalize=False"):
        fw.learn_network(form(good), abundances=True, normalize=False, **KINDS["fz_nz"])
    for bad, words in ((np.nan, "NaN"), (np.inf, "infinite"), (-np.inf, "infinite"), (-0.5, "negative")):
        for who, call in (("learn_network", lambda **kw: fw.learn_network(**KINDS["mi"], **kw)),
                          ("normalize_data", lambda **kw: fw.normalize_data(test_name="mi", **kw))):
            with pytest.raises(ValueError, match=r"%s: abundances=True: data holds .*%s" % (who, words)):
                call(data=form(_with(bad)), abundances=True)
            with pytest.raises(ValueError, match=r"%s: abundances=True: extra_data\[1\] holds .*%s" % (who, words)):
                call(data=form(good), extra_data=[(form(rel(counts(3, 5))), None), (form(_with(bad)), None)], abundances=True)
    # the host front-end of a dense table refuses them too: the option, not the routing, declares the values abundances
    with pytest.raises(ValueError, match="abundances=True: data holds a negative value"):
        fw.learn_network(_with(-0.5), abundances=True, device_normalize=False)
    assert recorded == [] and api_trace._LOG == []  # no front-end and no engine call was made


def test_routing_that_stays_with_the_option_on(recorded):
    x = rel(counts())
    for kw in (dict(device_normalize=False), dict(prec=64)):
        r = fw.learn_network(x, abundances=True, **KINDS["fz_nz"], **kw)  # dense: the host front-end, as today
        assert recorded == [] and r["counters"]["normalized_on_device"] is False and r["parameters"]["abundances"] is True
    with pytest.raises(ValueError, match="sparse data with device_normalize=False is not supported"):
        fw.learn_network(sp.csc_matrix(x), abundances=True, device_normalize=False)
    with pytest.raises(ValueError, match="sparse data with prec=64 is not supported"):
        fw.normalize_data(sp.csc_matrix(x), abundances=True, prec=64)
    assert recorded == []


def test_default_routing_is_unchanged(recorded):
    x = rel(counts())
    with pytest.raises(ValueError, match="needs integer counts in 0 .. 2\\^31 - 1: the device front-end takes nothing else"):
        fw.learn_network(sp.csc_matrix(x), **KINDS["fz_nz"])
    with pytest.raises(ValueError, match="needs integer counts"):
        fw.normalize_data(sp.csc_matrix(x), abundances=False)
    assert recorded == [] and api_trace._LOG == []
    r = fw.learn_network(x, **KINDS["fz_nz"])  # dense floats without the option: preprocess.normalize
    assert recorded == [] and r["counters"]["normalized_on_device"] is False
    # integer counts with the option off: the count front-end
    ints = fw.learn_network(counts(), **KINDS["fz_nz"])
    assert [c[0] for c in recorded] == ["normalize_counts"]
    # the key lists: without the option those of a call on an integer table, with it one more parameter
    assert list(r["parameters"]) == list(ints["parameters"]) and list(r["counters"]) == list(ints["counters"])
    on = fw.learn_network(x, abundances=True, **KINDS["fz_nz"])
    assert list(on["parameters"]) == list(ints["parameters"]) + ["abundances"] and on["parameters"]["abundances"] is True
    assert list(on["counters"]) == list(ints["counters"])
    truthy = fw.learn_network(x, abundances=1, **KINDS["fz_nz"])
    assert truthy["parameters"]["abundances"] is True


def test_the_keyword_joins_the_digest_of_a_distributed_run(monkeypatch):
    seen = []
    monkeypatch.setattr(fw.api, "_distributed_world", lambda: (None, 0, 2))
    monkeypatch.setattr(fw.api, "_distributed_input_check", lambda dist, rank, world, prec, device, tables, keywords: seen.append(keywords))
    class Stop(Exception):
        pass

    def stop(*a, **k):  # (the digest is taken first: the run ends at the table stage)
        raise Stop
    monkeypatch.setattr(fw.api, "_prepare_tables", stop)
    for flag in (False, True):
        with pytest.raises(Stop):
            fw.learn_network(rel(counts()), distributed=True, abundances=flag)
    assert [k["abundances"] for k in seen] == [False, True]


def test_the_anchor_sample_does_not_hang_on_the_summation_order():
    """clr_adapt anchors its pseudo-counts on the deepest sample.  Every sample of a relative-abundance table sums to 1 up to rounding,
    so the plain argmax of the Float64 sums -- the default of preprocess.adaptive_clr, and the reference's findmax -- is decided by
    the order of the additions: with the columns permuted it picks another sample and every value of the table moves (asserted
    below: the default stays that rule).  tie_anchor=True, what abundances=True asks for: sums within width * 2^-52 of the largest
    take part and the first such sample is the anchor, so the permuted table gives the permuted result, to a few Float32 ulps (the
    row's Sigma log is added in another order)."""
    rng = np.random.default_rng(0)
    c = rng.poisson(3.0, (40, 30)) * (rng.random((40, 30)) < 0.6)
    c[:, 0] += 1
    x, perm = rel(c), rng.permutation(30)
    assert np.argmax(x.sum(axis=1)) != np.argmax(x[:, perm].sum(axis=1))  # what the plain rule hangs on
    a, arm, acm = pre.normalize(x, "fz", tie_anchor=True)
    b, brm, bcm = pre.normalize(x[:, perm], "fz", tie_anchor=True)
    assert acm.all() and bcm.all() and np.array_equal(arm, brm)
    assert np.allclose(a[:, perm], b, rtol=1e-6, atol=1e-6), np.abs(a[:, perm] - b).max()
    assert not np.allclose(pre.normalize(x, "fz")[0][:, perm], pre.normalize(x[:, perm], "fz")[0], rtol=1e-3, atol=1e-3)
    # the default is the plain rule, spelled out: the anchor is np.argmax of the sums
    M = pre.filter_by_variance(x)[0]
    plain = pre.adaptive_clr(M)[0]
    first = pre.adaptive_clr(np.concatenate([M[[int(np.argmax(M.sum(axis=1)))]], M]), tie_anchor=True)[0][1:]  # that sample put first
    assert np.array_equal(plain, first)
    # counts: sums are exact, either rule is the same rule
    assert np.array_equal(pre.normalize(c, "fz")[0], pre.normalize(c, "fz", tie_anchor=True)[0])


def test_only_the_option_asks_for_the_tolerant_anchor(recorded, monkeypatch):
    seen, host = [], pre.normalize
    monkeypatch.setattr(pre, "normalize", lambda *a, **kw: seen.append(kw) or host(*a, **kw))
    x = rel(counts())
    fw.learn_network(x, **KINDS["fz"])  # a real-valued dense table without the option: the host front-end exactly as before
    fw.normalize_data(x, test_name="fz")
    assert seen == [dict(prec=32)] * 2
    del seen[:]
    fw.learn_network(x, abundances=True, device_normalize=False, **KINDS["fz"])  # the host route of the option: the device's rule
    fw.normalize_data(x, test_name="fz", abundances=True, prec=64)
    assert seen == [dict(prec=32, tie_anchor=True), dict(prec=64, tie_anchor=True)] and recorded == []
