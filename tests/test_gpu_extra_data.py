"""learn_network(extra_data=...) on the device: several count tables of the same samples, normalised apart and combined
(preprocess.combine_data), against the pieces it is composed of.  Shapes: n = 80 samples, p = 30 / 20 / 12 (the single_il schedule),
one sample emptied in the main table and another in the first extra table (the last table has a few empty samples of its own)."""
import functools
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import io as fio
from flashweave_jl_amd import synth

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:[0-9]+ samples had only zero counts")]

def _kw(sensitive, heterogeneous, **more):
    """max_k 3 for the Fisher-z tests; 1 for the discrete ones: their automatic n_obs_min is hps * 4 * min(levels^max_k, 8)
    (learning.jl:51-57), 40 / 60 at max_k 1 and 80 / 160 beyond, and the combined tables keep 74 or 75 of the 80 samples"""
    return dict(sensitive=sensitive, heterogeneous=heterogeneous, max_k=3 if sensitive else 1, **more)


MODES = [(True, False, "fz"), (True, True, "fz_nz"), (False, False, "mi"), (False, True, "mi_nz")]
N = 80


@functools.lru_cache(maxsize=None)
def _tables(sensitive, heterogeneous):
    """-> (main, header), [(extra, header), (extra, header)]; never written to"""
    out = []
    for tag, p, seed in (("m", 30, 21), ("a", 20, 22), ("b", 12, 23)):
        # (no habitats: with 12 columns a habitat-wise absent block empties half the samples; the tables are 40-55 % zeros as they are)
        c = synth.generate(p, N, seed, mode="S" if sensitive else "F")
        out.append((c, ["%s%d" % (tag, j) for j in range(p)]))
    out[0][0][11, :] = 0
    out[1][0][47, :] = 0
    for c, _ in out:
        c.setflags(write=False)
    return out[0], out[1:]


def _common(sensitive, heterogeneous):
    """the samples every table keeps, from the counts: a sample needs a read in a column that varies (preprocessing.jl:367-409)"""
    (main, _), extra = _tables(sensitive, heterogeneous)
    keep = np.ones(N, dtype=bool)
    for c in [main] + [t for t, _ in extra]:
        keep &= c[:, c.var(axis=0) > 0].sum(axis=1) > 0
    assert not keep[11] and not keep[47] and 60 <= keep.sum() <= N - 2
    return keep


def _same_network(a, b, tag):
    assert a["variable_ids"] == b["variable_ids"], tag
    assert a["meta_variable_mask"] == b["meta_variable_mask"], tag
    assert set(a["edges"]) == set(b["edges"]), tag
    assert all(a["edges"][e] == b["edges"][e] for e in a["edges"]), tag  # the same Float64, to the bit


@pytest.mark.parametrize("sensitive, heterogeneous, name", MODES)
def test_learn_network_is_normalize_data_plus_the_engine(sensitive, heterogeneous, name):
    (main, header), extra = _tables(sensitive, heterogeneous)
    kw = _kw(sensitive, heterogeneous)
    common = _common(sensitive, heterogeneous)
    with pytest.warns(UserWarning, match="^%d samples had only zero counts" % (N - common.sum())):
        net = fw.learn_network(main, header=header, extra_data=extra, **kw)
    nd = fw.normalize_data(main, extra, test_name=name, header=header)
    _same_network(net, fw.learn_network(nd["data"], normalize=False, header=nd["header"], **kw), name)
    # the layout: last extra table, first extra table, main; the samples every table kept
    ids = net["variable_ids"]
    assert [h[0] for h in ids] == sorted((h[0] for h in ids), key="bam".index) and {h[0] for h in ids} == set("bam")
    assert nd["data"].shape == (common.sum(), len(ids)) and np.array_equal(nd["row_mask"], common)
    assert not any(net["meta_variable_mask"]) and len(net["meta_variable_mask"]) == len(ids)
    assert net["counters"]["n_tables"] == 3 and net["parameters"]["extra_data"] == 2
    assert net["counters"]["normalized_on_device"] is True and net["counters"]["t_normalize_s"] > 0
    assert net["parameters"]["schedule"].startswith("single_il")
    print(name, "columns", len(ids), "edges", len(net["edges"]))
    if sensitive:
        assert len(net["edges"]) > 0  # (synth's AR(1) blocks: a Fisher-z network of 80 samples is not empty)
    # one table: nothing else changes
    one = fw.learn_network(main, header=header, **kw)
    assert one["counters"]["n_tables"] == 1 and one["parameters"]["extra_data"] == 0 and one["variable_ids"][0][0] == "m"


@pytest.mark.parametrize("sensitive, heterogeneous, name", MODES)
def test_device_front_end_against_host_front_end(sensitive, heterogeneous, name):
    (main, header), extra = _tables(sensitive, heterogeneous)
    dev = fw.normalize_data(main, extra, test_name=name, header=header)
    host = fw.normalize_data(main, extra, test_name=name, header=header, device_normalize=False)
    assert dev["header"] == host["header"]
    assert np.array_equal(dev["row_mask"], host["row_mask"]) and np.array_equal(dev["meta_mask"], host["meta_mask"])
    assert dev["data"].shape == host["data"].shape
    if name in ("mi", "mi_nz"):
        assert np.array_equal(dev["data"], host["data"])
    else:  # the bounds of tests/test_gpu_norm.py for one table: a combined table is columns of single tables
        diff = np.abs(dev["data"] - host["data"])
        print(name, "largest difference", diff.max(), "equal entries", (dev["data"] == host["data"]).mean())
        assert np.allclose(dev["data"], host["data"], rtol=2.4e-7, atol=1e-7), diff.max()


@pytest.mark.parametrize("sensitive, heterogeneous, name", [m for m in MODES if m[1]])
def test_sparse_tables_give_the_dense_tables_network(sensitive, heterogeneous, name):
    (main, header), extra = _tables(sensitive, heterogeneous)
    kw = _kw(sensitive, heterogeneous, header=header)
    dense = fw.learn_network(main, extra_data=extra, **kw)
    sparse_extra = [(sp.csc_matrix(t), h) for t, h in extra]
    sparse = fw.learn_network(sp.csc_matrix(main), extra_data=sparse_extra, **kw)
    _same_network(dense, sparse, name)
    assert sparse["counters"]["sparse_input"] is True and sparse["counters"]["n_tables"] == 3
    nd, ns = fw.normalize_data(main, extra, test_name=name), fw.normalize_data(sp.csc_matrix(main), sparse_extra, test_name=name)
    assert sp.issparse(ns["data"]) and ns["data"].toarray().tobytes() == np.ascontiguousarray(nd["data"]).tobytes()
    if name == "fz_nz":  # the CSC-resident layout only looks at the combined triple
        res = fw.learn_network(sp.csc_matrix(main), extra_data=sparse_extra, csc_resident=True, **kw)
        _same_network(dense, res, "csc_resident")
        assert res["counters"]["csc_resident"] is True and res["counters"]["n_tables"] == 3


@pytest.mark.parametrize("sensitive, heterogeneous, name", [MODES[0], MODES[3]])
def test_prepared_tables_are_only_laid_side_by_side(sensitive, heterogeneous, name):
    # normalize=False (learning.jl:537-541): no filter, no alignment, extra tables first
    (main, header), extra = _tables(sensitive, heterogeneous)
    common = _common(sensitive, heterogeneous)
    mats = []
    for t, _ in [(main, header)] + extra:
        m, rm, _ = fw.normalize_counts(t, name)
        mats.append(np.ascontiguousarray(m[common[rm]]))  # the gather, by hand
    assert all(m.shape[0] == common.sum() for m in mats)
    hdrs = [["%s%d" % (tag, j) for j in range(m.shape[1])] for tag, m in zip("mab", mats)]
    kw = _kw(sensitive, heterogeneous, normalize=False)
    with warnings.catch_warnings():
        warnings.filterwarnings("error", message=".*samples had only zero counts")  # nothing is dropped: nothing to warn about
        net = fw.learn_network(mats[0], header=hdrs[0], extra_data=[(mats[1], hdrs[1]), (mats[2], hdrs[2])], **kw)
    exp = fw.learn_network(np.hstack([mats[2], mats[1], mats[0]]), header=hdrs[2] + hdrs[1] + hdrs[0], **kw)
    _same_network(net, exp, name)
    assert net["counters"]["n_tables"] == 3 and net["counters"]["normalized_on_device"] is False
    # and that is the matrix normalize=True builds from the counts: the same edges
    assert net["edges"] == fw.learn_network(main, header=header, extra_data=extra, **dict(kw, normalize=True))["edges"]


def test_meta_data_belongs_to_the_main_table():
    (main, header), extra = _tables(False, True)
    meta = (np.arange(N) % 3 == 0).astype(np.float64)[:, None]
    net = fw.learn_network(main, header=header, extra_data=extra, meta_data=meta, meta_header=["M"], **_kw(False, True))
    nd = fw.normalize_data(main, extra, test_name="mi_nz", header=header, meta_data=meta, meta_header=["M"])
    assert net["variable_ids"] == nd["header"] and net["variable_ids"][-1] == "M" and net["variable_ids"][-2][0] == "m"
    assert net["meta_variable_mask"] == [False] * (len(nd["header"]) - 1) + [True] and nd["meta_mask"].tolist() == net["meta_variable_mask"]
    # the column followed the samples: the meta values of the common samples, as levels
    rows = nd["row_mask"]
    assert np.array_equal(rows, _common(False, True)) and np.array_equal(nd["data"][:, -1] != nd["data"][:, -1].min(), meta[rows, 0] == 1)


def test_path_form_equals_array_form(tmp_path):
    (main, header), extra = _tables(True, False)
    paths = [str(tmp_path / "main.tsv"), str(tmp_path / "its.csv"), tmp_path / "third.tsv"]
    for path, (tab, hdr) in zip(paths, [(main, header)] + extra):
        fio.write_table(str(path), tab, hdr)
    arrays = fw.learn_network(main, header=header, extra_data=extra)
    _same_network(arrays, fw.learn_network(paths), "paths")
    # one path, a meta data file, transposed files
    meta = (np.arange(N) % 3 == 0).astype(np.float64)[:, None]
    fio.write_table(str(tmp_path / "meta.tsv"), meta, ["M"])
    with_meta = fw.learn_network(paths[0], str(tmp_path / "meta.tsv"))
    _same_network(with_meta, fw.learn_network(main, header=header, meta_data=meta, meta_header=["M"]), "meta path")
    assert with_meta["variable_ids"][-1] == "M" and with_meta["meta_variable_mask"][-1] is True
    tpaths = [str(tmp_path / ("t%d.tsv" % i)) for i in range(3)]
    for path, (tab, hdr) in zip(tpaths, [(main, header)] + extra):
        fio.write_table(path, tab.T, row_ids=hdr)
    _same_network(arrays, fw.learn_network(tpaths, transposed=True), "transposed")
