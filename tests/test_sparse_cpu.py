"""Sparse (CSC) count tables, the part that needs no device: the as_csc helper, the refusals of learn_network (raised before any
device call, so nothing is mocked), and the two new entry points of the C ABI (exported, ABI still 6, argument errors)."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd.engine import as_csc


def _table(seed=0, n=40, p=12, fill=0.3):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 50, (n, p)) * (rng.random((n, p)) < fill)).astype(np.int64)


def _same(t, ref):
    assert t[3] == ref.shape
    assert t[0].dtype == np.int64 and t[1].dtype == np.int32
    assert np.array_equal(t[0], ref.indptr) and np.array_equal(t[1], ref.indices) and np.array_equal(t[2], ref.data)


def test_as_csc_canonical_triple_from_every_format():
    X = _table()
    ref = sp.csc_matrix(X.astype(np.int32))
    ref.sort_indices()
    for m in (sp.coo_matrix(X), sp.csr_matrix(X), sp.csc_matrix(X), sp.csc_array(X), sp.lil_matrix(X)):
        t = as_csc(m, np.int32)
        assert t[2].dtype == np.int32
        _same(t, ref)
    # unsorted CSC with duplicates (two halves that sum to the table) and explicit zeros
    rng = np.random.default_rng(1)
    i, j = np.nonzero(X)
    half = X[i, j] // 2
    zi, zj = np.nonzero(X == 0)
    rows = np.concatenate([i, i, zi[:7]])
    cols = np.concatenate([j, j, zj[:7]])
    vals = np.concatenate([half, X[i, j] - half, np.zeros(7, np.int64)])
    perm = rng.permutation(rows.size)
    rows, cols, vals = rows[perm], cols[perm], vals[perm]
    order = np.argsort(cols, kind="stable")  # column-major, rows in random order inside a column
    colptr = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=X.shape[1]))])
    _same(as_csc((colptr, rows[order], vals[order], X.shape), np.int32), ref)
    messy = sp.csc_matrix((vals[order], rows[order], colptr), shape=X.shape)
    assert not messy.has_sorted_indices or messy.nnz > ref.nnz
    _same(as_csc(messy, np.int32), ref)
    # float values that are integral are counts too; a float dtype keeps fractions
    _same(as_csc(sp.csr_matrix(X.astype(np.float64)), np.int32), ref)
    f = as_csc(sp.csr_matrix(X * 0.5), np.float32)
    assert f[2].dtype == np.float32 and np.array_equal(f[2], (ref.data * 0.5).astype(np.float32))


def test_as_csc_rejects_what_is_not_a_count():
    X = _table().astype(np.float64)
    for bad in (-1.0, 0.5, 2.0**31, np.inf):
        Y = X.copy()
        Y[3, 4] = bad
        with pytest.raises(ValueError):
            as_csc(sp.csc_matrix(Y), np.int32)
    Z = sp.csc_matrix(_table())
    Z.data = Z.data.astype(np.int64)
    Z.data[0] = 2**31
    with pytest.raises(ValueError):
        as_csc(Z, np.int32)
    Z.data[0] = 2**31 - 1
    assert as_csc(Z, np.int32)[2].max() == 2**31 - 1
    with pytest.raises(ValueError):
        as_csc(np.zeros((3, 3)), np.int32)  # dense arrays are not its business


@pytest.mark.parametrize("kwargs, name", [
    (dict(device_normalize=False), "device_normalize"),
    (dict(prec=64), "prec"),
    (dict(meta_data=np.ones((40, 1))), "meta_data"),
    (dict(sensitive=True, heterogeneous=False, normalize=False), "normalize=False"),
])
def test_learn_network_refuses_by_name(kwargs, name):
    with pytest.raises(ValueError) as ei:
        fw.learn_network(sp.csc_matrix(_table()), **kwargs)
    assert name in str(ei.value) and "sparse" in str(ei.value)


@pytest.mark.parametrize("bad", [0.5, -2.0, 2.0**31])
def test_learn_network_refuses_non_counts_when_normalizing(bad):
    Y = _table().astype(np.float64)
    Y[0, 0] = bad
    with pytest.raises(ValueError) as ei:
        fw.learn_network(sp.csc_matrix(Y), sensitive=False, heterogeneous=True, normalize=True)
    assert "normalize" in str(ei.value)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fw.lib_path()):
        fw.build_library()
    return fw.load_library()


def test_new_symbols_exported_and_abi_unchanged(lib):
    raw = ctypes.CDLL(fw.lib_path())
    assert hasattr(raw, "fw_normalize_counts_csc") and hasattr(raw, "fw_set_data_csc_f32")
    assert lib.fw_abi_version() == 6
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "flashweave_amd.h")).read()
    assert "int fw_normalize_counts_csc(" in hdr and "int fw_set_data_csc_f32(" in hdr


def test_argument_errors_need_no_device(lib):
    FW_ERR_ARG = -1
    colptr = np.array([0, 1, 2], np.int64)
    rowval = np.array([0, 1], np.int32)
    nzval = np.array([3, 4], np.int32)
    ocp, orow, oi = np.zeros(3, np.int64), np.zeros(2, np.int32), np.zeros(2, np.int32)
    rm, cm = np.zeros(2, np.uint8), np.zeros(2, np.uint8)
    no, po, nz = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None

    def call(n=2, p=2, kind=fw.FW_MI_NZ, colptr=colptr, rowval=rowval, nzval=nzval, ocp=ocp, oi=oi, rm=rm):
        return lib.fw_normalize_counts_csc(0, kind, n, p, P(colptr), P(rowval), P(nzval), P(ocp), P(orow), P(oi), None, P(rm), P(cm),
                                           ctypes.byref(no), ctypes.byref(po), ctypes.byref(nz))

    assert call(n=0) == FW_ERR_ARG and call(n=-3) == FW_ERR_ARG and call(p=0) == FW_ERR_ARG
    assert call(colptr=None) == FW_ERR_ARG and call(rowval=None) == FW_ERR_ARG and call(nzval=None) == FW_ERR_ARG
    assert call(ocp=None) == FW_ERR_ARG and call(oi=None) == FW_ERR_ARG and call(rm=None) == FW_ERR_ARG
    assert call(kind=9) == FW_ERR_ARG
    assert call(colptr=np.array([1, 1, 2], np.int64)) == FW_ERR_ARG  # does not start at 0
    assert call(colptr=np.array([0, 1, -2], np.int64)) == FW_ERR_ARG
    assert b"fw_normalize_counts_csc" in lib.fw_last_error(None)
    assert lib.fw_set_data_csc_f32(None, P(colptr), P(rowval), P(nzval.astype(np.float32))) == FW_ERR_ARG  # NULL context
