"""learn_network(extra_data=...) / normalize_data / the path form, the parts that need no device: preprocess.combine_data against a
restatement of the reference's combine_data (preprocessing.jl:596-635) written here, dense and CSC; the property the feature exists
for (tables normalised apart differ from the stacked table normalised once); every refusal, which all happen before any device call."""
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import io as fio
from flashweave_jl_amd import preprocess as pre

N = 12


def _counts():
    """main (p = 5) and two extra tables (p = 4, 3) of the same 12 samples; sample 2 has no reads in the first extra table, sample
    7 none in the main one"""
    rng = np.random.default_rng(5)
    main, e1, e2 = (rng.poisson(4.0, size=(N, p)) * (rng.random((N, p)) < 0.8) + (np.arange(p) == 0) for p in (5, 4, 3))
    e1[2, :] = 0
    main[7, :] = 0
    return main, e1, e2


def _normalised(test_name):
    """every table through the host front-end on its own -> tables, headers, row masks in combine_data's order (extras, main last)"""
    main, e1, e2 = _counts()
    tabs, hdrs, masks = [], [], []
    for tag, c in (("a", e1), ("b", e2), ("m", main)):
        d, rm, cm = pre.normalize(c, test_name)
        tabs.append(d), masks.append(rm)
        hdrs.append(["%s%d" % (tag, j) for j in np.nonzero(cm)[0]])
    return tabs, hdrs, masks


def _restated(tabs, hdrs, meta_masks, masks):
    """combine_data as the reference writes it: the common mask, indexin over sample numbers, pushfirst! of every extra table"""
    common = np.ones(N, dtype=bool)
    for m in masks:
        common &= m
    want = np.nonzero(common)[0]
    cols, names, meta = [], [], []
    for i, t in enumerate(tabs):
        have = list(np.nonzero(masks[i])[0])
        block = t[[have.index(s) for s in want], :]
        mm = np.zeros(t.shape[1], bool) if i < len(tabs) - 1 else np.asarray(meta_masks[i])
        if i == len(tabs) - 1:
            cols.append(block), names.append(hdrs[i]), meta.append(mm)
        else:
            cols.insert(0, block), names.insert(0, hdrs[i]), meta.insert(0, mm)
    return np.hstack(cols), sum(names, []), np.concatenate(meta), common


@pytest.mark.parametrize("test_name", ["fz", "fz_nz", "mi", "mi_nz"])
def test_combine_data_equals_the_restatement(test_name):
    tabs, hdrs, masks = _normalised(test_name)
    main_meta = np.zeros(tabs[2].shape[1], bool)
    main_meta[-1] = True  # (as if the main table's last column were a meta variable)
    with pytest.warns(UserWarning, match="2 samples"):
        got = pre.combine_data(tabs, hdrs, [None, None, main_meta], masks)
    exp = _restated(tabs, hdrs, [None, None, main_meta], masks)
    assert got[0].dtype == exp[0].dtype and got[0].shape == exp[0].shape == (10, sum(t.shape[1] for t in tabs))
    assert got[0].tobytes() == np.ascontiguousarray(exp[0]).tobytes() or np.array_equal(got[0], exp[0])
    assert np.array_equal(got[0], exp[0])
    assert got[1] == exp[1] and got[1][0].startswith("b") and got[1][tabs[1].shape[1]].startswith("a") and got[1][-1].startswith("m")
    assert np.array_equal(got[2], exp[2]) and got[2].sum() == 1 and got[2][-1]
    assert np.array_equal(got[3], exp[3]) and not got[3][2] and not got[3][7] and got[3].sum() == 10
    # the gathered rows: table a kept samples 0,1,3..11, the main table 0..6,8..11; both lose one more row
    a0 = tabs[1].shape[1]
    assert np.array_equal(got[0][:, a0:a0 + tabs[0].shape[1]], tabs[0][[i for i, s in enumerate(np.nonzero(masks[0])[0]) if s != 7]])


@pytest.mark.parametrize("test_name", ["fz_nz", "mi", "mi_nz"])
@pytest.mark.parametrize("form", ["scipy", "triple"])
def test_combine_data_csc_equals_dense_bytewise(test_name, form):
    tabs, hdrs, masks = _normalised(test_name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        dense = pre.combine_data(tabs, hdrs, [None] * 3, masks)
        csc = [sp.csc_matrix(t) for t in tabs]
        if form == "triple":
            csc = [(m.indptr, m.indices, m.data, m.shape) for m in csc]
        got = pre.combine_data(csc, hdrs, [None] * 3, masks)
    assert sp.issparse(got[0]) and got[0].format == "csc" and got[0].dtype == dense[0].dtype
    assert got[0].toarray().tobytes() == np.ascontiguousarray(dense[0]).tobytes()
    assert got[0].has_sorted_indices and got[1] == dense[1] and np.array_equal(got[2], dense[2]) and np.array_equal(got[3], dense[3])


def test_combine_data_csc_keeps_stored_zeros():
    # a stored 0.0 of clr_nz is a present count whose value is 0: the gather and the stacking must not drop it
    a = sp.csc_matrix((3, 2), dtype=np.float32)
    a.indptr, a.indices, a.data = np.array([0, 2, 3], np.int32), np.array([0, 2, 1], np.int32), np.array([0.0, 1.5, 0.0], np.float32)
    b = sp.csc_matrix(np.array([[1.0], [2.0]], np.float32))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out = pre.combine_data([a, b], [["p", "q"], ["r"]], [None, None], [np.array([1, 1, 1], bool), np.array([1, 0, 1], bool)])[0]
    assert out.shape == (2, 3) and out.indptr.tolist() == [0, 2, 2, 4] and out.indices.tolist() == [0, 1, 0, 1]
    assert out.data.tolist() == [0.0, 1.5, 1.0, 2.0]


def test_combine_data_refuses_a_mix_and_wrong_lengths():
    tabs, hdrs, masks = _normalised("mi")
    with pytest.raises(ValueError, match="extra_data"):
        pre.combine_data([sp.csc_matrix(tabs[0]), tabs[1], tabs[2]], hdrs, [None] * 3, masks)
    with pytest.raises(ValueError, match="extra_data"):
        pre.combine_data(tabs, [hdrs[0][:-1], hdrs[1], hdrs[2]], [None] * 3, masks)
    with pytest.raises(ValueError, match="extra_data"):
        pre.combine_data([tabs[0][:-1], tabs[1], tabs[2]], hdrs, [None] * 3, masks)


def test_normalising_apart_is_not_normalising_the_stacked_table():
    """The reason the feature exists: clr divides a sample by the geometric mean of ITS OWN table.  Stacking first gives every sample
    one composition across experiments, so the same columns get other values."""
    main, e1, e2 = _counts()
    keep = np.ones(N, bool)
    keep[[2, 7]] = False  # (the stacked table has no empty sample: compare on the samples both forms keep)
    tabs, hdrs, masks = _normalised("fz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        apart = pre.combine_data(tabs, hdrs, [None] * 3, masks)[0]
    stacked, rm, cm = pre.normalize(np.hstack([e2, e1, main]), "fz")
    assert rm.all() and cm.all() and apart.shape[1] == stacked.shape[1]
    assert not np.allclose(apart, stacked[keep], rtol=1e-3, atol=1e-3)
    # every block of `apart` is centred on its own (clr rows sum to 0 within a table); the stacked table's blocks are not
    assert np.abs(apart[:, :3].sum(axis=1)).max() < 1e-4 and np.abs(stacked[keep][:, :3].sum(axis=1)).max() > 0.1


def test_normalize_data_host_front_end_is_the_composition():
    main, e1, e2 = _counts()
    with pytest.warns(UserWarning, match="2 samples"):
        r = fw.normalize_data(main, [(e1, None), (e2, list("xyz"))], test_name="mi_nz", header=list("ABCDE"), device_normalize=False)
    tabs, hdrs, masks = _normalised("mi_nz")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp = pre.combine_data(tabs, hdrs, [None] * 3, masks)
    assert np.array_equal(r["data"], exp[0]) and np.array_equal(r["row_mask"], exp[3]) and not r["meta_mask"].any()
    assert len(r["header"]) == r["data"].shape[1] and set(r["header"]) <= set("xyzABCDE") | {"X6", "X7", "X8", "X9"}
    assert r["header"][0] in "xyz" and r["header"][-1] in "ABCDE"
    # one table: the reference's first form
    one = fw.normalize_data(main, test_name="mi_nz", device_normalize=False)
    d, rm, cm = pre.normalize(main, "mi_nz")
    assert np.array_equal(one["data"], d) and np.array_equal(one["row_mask"], rm) and one["header"] == ["X%d" % (j + 1) for j in np.nonzero(cm)[0]]


def test_one_front_end_for_all_tables(monkeypatch):
    # a table of relative abundances sends EVERY table to the host front-end: one run never mixes two
    def no_device(*a, **k):
        raise AssertionError("the device front-end was reached")
    monkeypatch.setattr(fw.api, "normalize_counts", no_device)
    main, e1, e2 = _counts()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        r = fw.normalize_data(main, [(e1 / 3.0, None), (e2, None)], test_name="fz_nz")
    assert r["data"].shape[0] == 10


def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    monkeypatch.setattr(fw.api, "Engine", no_device)
    monkeypatch.setattr(fw.api, "normalize_counts", no_device)


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("extra, words", [
    (lambda m, a, b: [(a[:-1], None)], "rows"),                         # another number of samples
    (lambda m, a, b: [(a, ["h1", "h2"])], "header"),                    # a header of another length
    (lambda m, a, b: [(a, None), (sp.csc_matrix(b), None)], "sparse"),  # dense data, a sparse extra table
    (lambda m, a, b: [a], "pair"),                                      # a bare table
    (lambda m, a, b: [(a, None, None)], "pair"),                        # a triple
    (lambda m, a, b: [(a, "abcd")], "pair"),                            # a string where the header goes
    (lambda m, a, b: (a, None), "pair"),                                # one pair instead of a list of pairs
    (lambda m, a, b: {"a": a}, "list"),                                 # no list at all
])
def test_learn_network_refuses_by_name_before_any_device_call(extra, words, normalize, monkeypatch):
    _no_device(monkeypatch)
    main, e1, e2 = _counts()
    with pytest.raises(ValueError) as ei:
        fw.learn_network(main, extra_data=extra(main, e1, e2), sensitive=False, normalize=normalize)
    assert "extra_data" in str(ei.value) and words in str(ei.value)


def test_sparse_data_with_a_dense_extra_table_is_refused(monkeypatch):
    _no_device(monkeypatch)
    main, e1, e2 = _counts()
    with pytest.raises(ValueError) as ei:
        fw.learn_network(sp.csc_matrix(main), extra_data=[(e1, None)], sensitive=False)
    assert "extra_data" in str(ei.value) and "sparse" in str(ei.value)
    with pytest.raises(ValueError) as ei:
        fw.normalize_data(sp.csc_matrix(main), [(e1, None)], test_name="mi")
    assert "extra_data" in str(ei.value) and "sparse" in str(ei.value)
    # the refusals sparse data has today keep their wording with extra tables present
    with pytest.raises(ValueError, match="learn_network: sparse data with device_normalize=False is not supported"):
        fw.learn_network(sp.csc_matrix(main), extra_data=[(sp.csc_matrix(e1), None)], device_normalize=False)
    with pytest.raises(ValueError, match="learn_network: sparse data with prec=64 is not supported"):
        fw.learn_network(sp.csc_matrix(main), extra_data=[(sp.csc_matrix(e1), None)], prec=64)
    # a sparse extra table of relative abundances: what the main table is refused with
    with pytest.raises(ValueError, match="integer counts"):
        fw.learn_network(sp.csc_matrix(main), extra_data=[(sp.csc_matrix(e1 / 3.0), None)], sensitive=False)


def test_path_form_refusals(tmp_path, monkeypatch):
    _no_device(monkeypatch)
    main, e1, e2 = _counts()
    meta = str(tmp_path / "meta.tsv")
    fio.write_table(meta, np.arange(N)[:, None] % 2, ["M"])
    with pytest.raises(ValueError, match="meta_data_path"):
        fw.learn_network(main, meta)                       # an array with a meta data path
    with pytest.raises(ValueError, match="meta_data_path"):
        fw.learn_network(main, meta_data_path=meta)
    with pytest.raises(ValueError, match="transposed"):
        fw.learn_network(main, transposed=True)
    with pytest.raises(TypeError, match="meta_data_path"):
        fw.learn_network(str(tmp_path / "a.tsv"), False)   # an option passed by position
    # formats: what io.load_data raises, unchanged
    bad = tmp_path / "table.xlsx"
    bad.write_text("x")
    with pytest.raises(ValueError, match="load_data: unsupported format"):
        fw.learn_network(str(bad))
    good = str(tmp_path / "a.tsv")
    fio.write_table(good, main)
    with pytest.raises(ValueError, match="load_data: unsupported format"):
        fw.learn_network([good, bad])
    # a file with another number of samples is refused like an array
    short = tmp_path / "short.csv"
    fio.write_table(str(short), e1[:-1])
    with pytest.raises(ValueError, match="extra_data.*rows"):
        fw.learn_network([good, short])


def test_write_table_round_trips_through_load_data(tmp_path):
    main, e1, e2 = _counts()
    for name, tab in (("a.tsv", main), ("b.csv", e1 / 4.0)):
        path = str(tmp_path / name)
        fio.write_table(path, tab, ["v%d" % j for j in range(tab.shape[1])])
        data, header, meta, meta_header = fio.load_data(path)
        assert np.array_equal(data, tab) and header == ["v%d" % j for j in range(tab.shape[1])] and meta is None
    t = str(tmp_path / "t.tsv")
    fio.write_table(t, main.T)
    assert np.array_equal(fio.load_data(t, transposed=True)[0], main)


def test_the_keyword_exists():
    """On the parent commit extra_data falls into **unsupported and raises TypeError: the test that fails without the feature."""
    import inspect
    sig = inspect.signature(fw.learn_network).parameters
    assert sig["extra_data"].default is None and sig["meta_data_path"].default is None and sig["transposed"].default is False
    assert list(sig)[:2] == ["data", "meta_data_path"]
    main, e1, e2 = _counts()
    try:
        fw.learn_network(main, extra_data=[(e1, None), (e2, None)], sensitive=False, device_normalize=False)
    except TypeError as e:  # the parent: "unsupported options ['extra_data']"
        pytest.fail("learn_network does not take extra_data: %s" % e)
    except fw.FlashWeaveError:
        pass  # no device here: the tables were taken, normalised and combined, and the engine said what is missing
    assert callable(fw.normalize_data) and fw.normalize_data is fw.api.normalize_data
