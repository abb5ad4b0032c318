"""learn_network(meta_mask=...) on the device: meta variables inside the table, dense or sparse, against the existing meta_data path
(the OTU block and the meta block as two arguments).  Every comparison is exact: both sides run the same front-end and the same
engine on the same bytes.  The table is tests/meta_mask_table.py (200 samples, 48 OTUs + 4 meta columns at positions 3, 17, 30 and
last; tests/test_meta_mask_cpu.py checks on the CPU oracle that its networks hold meta edges and OTU edges in every mode);
max_k = 2, default round_size."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from tests.meta_mask_table import META_NAMES, SEED, edge_kinds, table

pytestmark = pytest.mark.gpu

MODES = [(True, False, "fz"), (True, True, "fz_nz"), (False, False, "mi"), (False, True, "mi_nz")]
_HET = {name: dict(sensitive=s, heterogeneous=h, max_k=2) for s, h, name in MODES}


@functools.lru_cache(maxsize=None)
def _existing(name, n=200, p_otu=48):
    """the path that exists: the OTU block with meta_data; computed once per mode, never written to"""
    full, mask, header, counts, meta = table(n, p_otu, SEED)
    return fw.learn_network(counts, meta_data=meta, header=[h for h, m in zip(header, mask) if not m], meta_header=META_NAMES, **_HET[name])


@functools.lru_cache(maxsize=None)
def _sparse(name):
    full, mask, header, _, _ = table()
    return fw.learn_network(sp.csc_matrix(full), meta_mask=mask, header=header, **_HET[name])


def _same_network(a, b, tag):
    assert a["variable_ids"] == b["variable_ids"], tag
    assert a["meta_variable_mask"] == b["meta_variable_mask"], tag
    assert set(a["edges"]) == set(b["edges"]), tag
    assert all(a["edges"][e] == b["edges"][e] for e in a["edges"]), tag  # the same Float64, to the bit


@pytest.mark.parametrize("sensitive, heterogeneous, name", MODES)
def test_dense_mask_form_is_the_meta_data_path(sensitive, heterogeneous, name):
    full, mask, header, _, _ = table()
    exp = _existing(name)
    # what makes the comparison mean something: the existing path's network holds meta edges and OTU edges
    with_meta, between_otus = edge_kinds(exp["edges"], exp["meta_variable_mask"])
    print(name, "edges with a meta endpoint", with_meta, "between OTUs", between_otus)
    assert with_meta >= 1 and between_otus >= 1
    assert exp["variable_ids"][-3:] == META_NAMES[:3] and exp["meta_variable_mask"] == [False] * 48 + [True] * 3
    got = fw.learn_network(full, meta_mask=mask, header=header, **_HET[name])
    _same_network(got, exp, name)
    assert got["counters"]["normalized_on_device"] is True and got["counters"]["sparse_input"] is False
    assert got["parameters"]["meta_mask"] == 4 and exp["parameters"]["meta_mask"] == 0
    assert got["parameters"]["schedule"].startswith("single_il")


@pytest.mark.parametrize("sensitive, heterogeneous, name", MODES)
def test_sparse_mask_form_is_the_meta_data_path(sensitive, heterogeneous, name):
    # the sparse table holds the non-integral covariate: it only gets past the count check because the split comes first
    full, mask, _, _, _ = table()
    assert np.any(full[:, mask] != np.floor(full[:, mask]))
    got = _sparse(name)
    _same_network(got, _existing(name), name)
    assert got["counters"]["sparse_input"] is True and got["counters"]["normalized_on_device"] is True
    assert got["parameters"]["meta_mask"] == 4


def test_csc_resident_on_the_combined_table():
    full, mask, header, _, _ = table()
    res = fw.learn_network(sp.csc_matrix(full), meta_mask=mask, header=header, csc_resident=True, **_HET["fz_nz"])
    _same_network(res, _sparse("fz_nz"), "csc_resident")
    nd = fw.normalize_data(sp.csc_matrix(full), test_name="fz_nz", header=header, meta_mask=mask)
    n, p = nd["data"].shape
    nnz = int(np.count_nonzero(nd["data"].data))
    # the single-OTU sample's clr_nz value is a stored 0.0f of the combined table: present for the front-end, no value != 0
    m, col = nd["data"], nd["header"].index("otu5")
    assert m.indices[m.indptr[col]] == 0 and m.data[m.indptr[col]] == 0.0 and m.nnz > nnz and (n, p) == (200, 51)
    assert res["counters"]["csc_resident"] is True
    assert res["counters"]["data_resident_bytes"] == 12 * p * ((n + 63) // 64) + 4 * nnz


def test_beyond_512_variables_the_device_rounds_run():
    full, mask, header, _, _ = table(256, 600, SEED)
    assert full.shape == (256, 604) and np.nonzero(mask)[0].tolist() == [3, 17, 30, 603]
    got = fw.learn_network(sp.csc_matrix(full), meta_mask=mask, header=header, **_HET["fz_nz"])
    exp = _existing("fz_nz", 256, 600)
    _same_network(got, exp, "600 OTUs")
    assert len(got["variable_ids"]) > 512 and got["parameters"]["schedule"].startswith("rounds of")
    assert got["parameters"]["schedule"] == exp["parameters"]["schedule"] and got["counters"]["sparse_input"] is True
    with_meta, between_otus = edge_kinds(got["edges"], got["meta_variable_mask"])
    print("600 OTUs: edges with a meta endpoint", with_meta, "between OTUs", between_otus)
    assert with_meta >= 1 and between_otus >= 1


@pytest.mark.parametrize("name", ["mi_nz", "fz_nz"])
def test_prepared_sparse_matrix_with_its_mask(name):
    # normalize=False: the normalised output of the sparse run (Int32 levels / Float32 values, CSC) goes in as it is, with the mask
    full, mask, header, _, _ = table()
    nd = fw.normalize_data(sp.csc_matrix(full), test_name=name, header=header, meta_mask=mask)
    assert sp.issparse(nd["data"]) and nd["data"].dtype == (np.int32 if name == "mi_nz" else np.float32)
    got = fw.learn_network(nd["data"], normalize=False, meta_mask=nd["meta_mask"], header=nd["header"], **_HET[name])
    _same_network(got, _sparse(name), name)
    assert got["parameters"]["meta_mask"] == 3 and got["counters"]["normalized_on_device"] is False
    assert got["counters"]["sparse_input"] is True
