"""normalize_data(norm_mode=...), the parts that need no device: the two total-sum-scaling modes on the host front-end against the
reference's fixtures (tests/golden/tss.tsv, tss_nonzero_binned.tsv; bit for bit), the four aliases, the refusals, the meta
variables, extra_data and prec=64.  Where a device front-end would run, fw.api.normalize_counts / normalize_abundances are
replaced by host stand-ins (tests/norm_mode_tables.host_stand_in; the recording one of tests/api_trace for the aliases)."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import preprocess as pre
from tests import api_trace
from tests.norm_mode_tables import ALIASES, TSS_MODES, bits, dense, f32_sum_left_to_right, fixture, hmp, host_stand_in

nd = fw.normalize_data


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(fw.api, "normalize_counts", host_stand_in)
    monkeypatch.setattr(fw.api, "normalize_abundances", host_stand_in)


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **kw):
        raise AssertionError("a device front-end was called")
    monkeypatch.setattr(fw.api, "normalize_counts", refuse)
    monkeypatch.setattr(fw.api, "normalize_abundances", refuse)


def test_the_keyword_exists(no_device):
    """Without the feature norm_mode is an unexpected keyword (TypeError)."""
    p = inspect.signature(nd).parameters
    assert p["norm_mode"].default is None and p["test_name"].default is None
    r = nd(api_trace.counts(), norm_mode="tss", device_normalize=False)
    assert r["data"].dtype == np.float32 and np.allclose(r["data"].sum(axis=1), 1.0, atol=1e-6)
    for f in (pre.normalize, fw.normalize_counts, fw.normalize_abundances):
        assert inspect.signature(f).parameters["norm"].default is None


@pytest.mark.parametrize("mode", TSS_MODES)
def test_host_front_end_gives_the_reference_fixture(mode, no_device):
    r = nd(hmp(), norm_mode=mode, device_normalize=False)
    exp = fixture(mode)
    assert exp.shape == (346, 50) and r["data"].shape == exp.shape and r["data"].dtype == exp.dtype
    assert np.array_equal(bits(r["data"]), bits(exp))
    assert int(r["row_mask"].sum()) == 346 and len(r["header"]) == 50 and not r["meta_mask"].any()


@pytest.mark.parametrize("mode", TSS_MODES)
@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_stand_in_front_end_gives_the_reference_fixture(mode, form, stand_in):
    table = sp.csr_matrix(hmp()) if form == "sparse" else hmp()
    r = nd(table, norm_mode=mode)
    exp = fixture(mode)
    assert sp.issparse(r["data"]) is (form == "sparse") and r["data"].dtype == exp.dtype  # (output in the input's format)
    assert np.array_equal(bits(dense(r["data"])), bits(exp))


def test_the_row_sum_is_taken_left_to_right():
    row = np.ones(40)
    row[0] = 2.0 ** 24  # every 1 added to 2^24 is rounded away; added first, the ones survive
    s = f32_sum_left_to_right(row)
    assert s == np.float32(2.0 ** 24) and s != np.float32(row.sum()) and s != f32_sum_left_to_right(row[::-1])
    got = pre.tss(np.stack([row, row[::-1]]))
    assert np.array_equal(bits(got[0]), bits(row.astype(np.float32) / s))
    assert np.array_equal(bits(got[1]), bits(row[::-1].astype(np.float32) / np.float32(2.0 ** 24 + 39)))


def _traced(monkeypatch, call):
    monkeypatch.setattr(fw.api, "normalize_counts", api_trace._recording_front_end)
    del api_trace._LOG[:]
    r = call()
    return api_trace._rec(dict(r)), list(api_trace._LOG)


@pytest.mark.parametrize("mode", sorted(ALIASES))
@pytest.mark.parametrize("form", ["host", "dense", "sparse", "mask"])
def test_an_alias_is_the_test_name_call(mode, form, monkeypatch):
    table, kw = {"host": (api_trace.counts(), dict(device_normalize=False)), "dense": (api_trace.counts(), {}),
                 "sparse": (sp.csc_matrix(api_trace.counts()), {}),
                 "mask": (sp.csc_matrix(api_trace.masked()), dict(meta_mask=api_trace.MASK))}[form]
    by_mode = _traced(monkeypatch, lambda: nd(table, norm_mode=mode, **kw))
    by_name = _traced(monkeypatch, lambda: nd(table, test_name=ALIASES[mode], **kw))
    assert by_mode[1] == by_name[1] and len(by_mode[1]) == (0 if form == "host" else 1)  # the recorded front-end calls, keywords included
    assert api_trace.difference(by_mode[0], by_name[0]) is None and by_mode[0] == by_name[0]


def test_refusals_come_before_any_device_call(no_device):
    x = api_trace.counts()
    with pytest.raises(ValueError, match="test_name.*norm_mode"):
        nd(x, test_name="fz", norm_mode="tss")
    with pytest.raises(ValueError, match="test_name.*norm_mode"):
        nd(x, test_name="mi_nz", norm_mode="clr-nonzero-binned")  # (even where they agree)
    with pytest.raises(ValueError) as e:
        nd(x, norm_mode="rows")
    assert all(name in str(e.value) for name in list(ALIASES) + list(TSS_MODES)) and "norm_mode" in str(e.value)
    with pytest.raises(ValueError, match="unsupported test_name"):
        nd(x, test_name="tss")
    rel = x / x.sum(axis=1, keepdims=True)
    for mode in TSS_MODES:
        for bad in (2.0 ** -127, 2.0 ** 97):
            y = rel.copy()
            y[2, 3] = bad
            for table in (y, sp.csc_matrix(y)):
                with pytest.raises(ValueError, match="norm_mode.*abundances.* data holds"):
                    nd(table, norm_mode=mode, abundances=True)
                with pytest.raises(ValueError, match=r"norm_mode.*extra_data\[0\] holds"):
                    nd(sp.csc_matrix(rel) if sp.issparse(table) else rel, norm_mode=mode, abundances=True, extra_data=[(table, None)])
    for bad in (2.0 ** -127, 2.0 ** 97):  # the front-end of its own refuses them as well
        y = rel.copy()
        y[2, 3] = bad
        with pytest.raises(ValueError, match="normalize_abundances.*norm"):
            fw.normalize_abundances(y, "fz", norm="tss")
    for call in (lambda: fw.normalize_counts(x, "fz", norm="rows"), lambda: fw.normalize_counts(x, "mi", norm="tss"),
                 lambda: fw.normalize_abundances(rel, "fz", norm="tss-nonzero-binned"), lambda: pre.normalize(x, "fz_nz", norm="tss")):
        with pytest.raises(ValueError, match="norm"):
            call()


def test_the_bounds_are_taken(stand_in):
    rel = api_trace.counts() / api_trace.counts().sum(axis=1, keepdims=True)
    rel[2, 3], rel[1, 1] = 2.0 ** -126, 2.0 ** 96
    r = nd(rel, norm_mode="tss", abundances=True)
    assert np.isfinite(r["data"]).all() and (r["data"][rel != 0] >= 0).all()


META = np.stack([np.arange(6) % 2, [0.0, 0.25, 0.5, 1.5, 2.25, 3.5]], axis=1).astype(np.float64)  # a 0 / 1 column, a covariate with a zero


@pytest.mark.parametrize("how", ["meta_data", "meta_mask", "meta_mask_sparse"])
def test_meta_columns_under_the_tss_modes(how, stand_in):
    x = api_trace.counts()
    if how == "meta_data":
        call = lambda mode: nd(x, norm_mode=mode, meta_data=META, make_onehot=False, device_normalize=False)
    else:
        table = np.concatenate([x, META], axis=1)
        table = sp.csc_matrix(table) if how == "meta_mask_sparse" else table
        call = lambda mode: nd(table, norm_mode=mode, meta_mask=np.r_[np.zeros(8, bool), True, True])
    r = call("tss")  # a continuous norm: the meta columns as they are, nothing discretised, nothing shifted
    assert list(r["meta_mask"][-2:]) == [True, True] and r["data"].dtype == np.float32
    assert np.array_equal(dense(r["data"])[:, -2:], META.astype(np.float32))
    r = call("tss-nonzero-binned")  # a discrete norm: the covariate in two bins, the 0 / 1 column as it is -- no +1 shift
    got = dense(r["data"])[:, -2:]
    assert r["data"].dtype == np.int32 and np.array_equal(got[:, 0], META[:, 0])
    assert np.array_equal(got[:, 1], pre.discretize(META[:, 1], 2)) and set(got[:, 1]) == {0, 1}


@pytest.mark.parametrize("form", ["host", "dense", "sparse"])
def test_extra_data_has_its_own_row_sums(form, stand_in):
    main, extra = api_trace.counts(), 100 * api_trace.counts(4, 2)
    wrap = sp.csc_matrix if form == "sparse" else np.asarray
    r = nd(wrap(main), norm_mode="tss", extra_data=[(wrap(extra), None)], device_normalize=(form != "host"))
    got = dense(r["data"])
    e, m = pre.normalize(extra, "fz", norm="tss")[0], pre.normalize(main, "fz", norm="tss")[0]
    assert np.array_equal(bits(got), bits(np.concatenate([e, m], axis=1)))  # [extra, main], each over its own sums
    assert np.allclose(got[:, :e.shape[1]].sum(axis=1), 1.0, atol=1e-6) and np.allclose(got[:, e.shape[1]:].sum(axis=1), 1.0, atol=1e-6)
    r = nd(wrap(main), norm_mode="tss-nonzero-binned", extra_data=[(wrap(extra), None)], device_normalize=(form != "host"))
    e, m = pre.normalize(extra, "mi_nz", norm="tss-nonzero-binned")[0], pre.normalize(main, "mi_nz", norm="tss-nonzero-binned")[0]
    assert np.array_equal(dense(r["data"]), np.concatenate([e, m], axis=1)) and r["data"].dtype == np.int32


def test_prec64_is_the_same_rule_in_float64(no_device):
    r64, r32 = nd(hmp(), norm_mode="tss", prec=64), nd(hmp(), norm_mode="tss", device_normalize=False)
    a64, a32 = r64["data"], r32["data"]
    assert a64.dtype == np.float64 and a64.shape == a32.shape == (346, 50)
    assert (np.abs(a64.astype(np.float32) - a32) <= np.spacing(a32)).all()  # within one ulp of the Float32 result
    x = hmp()[r64["row_mask"]].astype(np.float64)
    s = np.zeros(x.shape[0])
    for j in range(x.shape[1]):
        s = s + x[:, j]
    assert np.array_equal(bits(a64), bits(x / s[:, None]))  # (all 50 columns are kept)
    b64 = nd(hmp(), norm_mode="tss-nonzero-binned", prec=64)["data"]
    assert b64.dtype == np.int32 and set(np.unique(b64)) == {0, 1, 2}
