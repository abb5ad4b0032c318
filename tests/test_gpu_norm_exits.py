"""Every refusal of the device normalisation front-end that leaves AFTER device memory is held (csrc/fw_norm.hip), through the raw
entry points like test_gpu_abund._raw: the status, the whole message as the source prints it, and a good call right afterwards in
the same process that returns the bytes it returned before.

Two such exits cannot be reached with arguments the entry points accept and are left out: "no sample has reads" (a kept column is
not constant, so it holds a positive value and its sample has reads) and "samples with all zero abundances are not allowed" (a
sample with reads holds a non-zero in a kept column, and so does the anchor)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import engine

pytestmark = pytest.mark.gpu

FW_ERR_ARG = -1
ENTRY = {(np.int32, False): "fw_normalize_counts", (np.int32, True): "fw_normalize_counts_csc",
         (np.float64, False): "fw_normalize_abund", (np.float64, True): "fw_normalize_abund_csc"}
GOOD = np.array([[4, 0, 1, 7], [0, 3, 2, 7], [5, 1, 0, 2], [2, 2, 6, 0], [1, 0, 3, 3]])


def _raw(kind, x, dtype, sparse):
    """the entry point for (dtype, sparse) on the values exactly as given -> (rc, message, entry point's name)"""
    L = fw.load_library()
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    n, p = x.shape
    rm, cm, no, po, nz = np.zeros(n, np.uint8), np.zeros(p, np.uint8), C.c_int32(0), C.c_int32(0), C.c_int64(0)
    oi, of = np.zeros(n * p, np.int32), np.zeros(n * p, np.float32)
    name = ENTRY[dtype, sparse]
    if not sparse:
        v = np.asfortranarray(x, dtype=dtype)
        rc = getattr(L, name)(0, kind, n, p, P(v), P(of), P(oi), P(rm), P(cm), C.byref(no), C.byref(po))
    else:
        present = ~(x == 0)  # (a NaN is a stored entry)
        cols, rows = np.nonzero(present.T)
        cp = np.concatenate(([0], np.cumsum(present.sum(axis=0)))).astype(np.int64)
        rv, v = rows.astype(np.int32), np.ascontiguousarray(x[rows, cols], dtype=dtype)
        ocp, orow = np.zeros(p + 1, np.int64), np.zeros(n * p, np.int32)
        rc = getattr(L, name)(0, kind, n, p, P(cp), P(rv), P(v), P(ocp), P(orow), P(oi), P(of), P(rm), P(cm), C.byref(no), C.byref(po),
                              C.byref(nz))
    return rc, L.fw_last_error(None).decode(), name


def _good(dtype, sparse):
    """a good call of the same entry point -> its bytes"""
    front_end = engine.normalize_counts if dtype is np.int32 else engine.normalize_abundances
    out, rm, cm = front_end(sp.csc_matrix(GOOD) if sparse else GOOD, "mi_nz")
    parts = (out.data, out.indices, out.indptr) if sparse else (np.asfortranarray(out),)
    return [np.asarray(a).tobytes(order="F") for a in parts] + [rm.tobytes(), cm.tobytes()]


def _refused(kind, x, dtype, sparse, words):
    before = _good(dtype, sparse)
    rc, msg, name = _raw(kind, np.array(x, dtype=np.float64), dtype, sparse)
    assert rc == FW_ERR_ARG, (rc, msg)
    assert msg == "%s: %s" % (name, words)
    assert _good(dtype, sparse) == before


FORMS = pytest.mark.parametrize("dtype,sparse", list(ENTRY), ids=list(ENTRY.values()))


@FORMS
def test_every_column_is_constant(dtype, sparse):
    _refused(engine.FW_FZ_NZ, [[3, 3], [3, 3]], dtype, sparse, "every column is constant")


@FORMS
def test_no_column_with_two_levels(dtype, sparse):
    _refused(engine.FW_MI, [[1, 2], [2, 1], [3, 5]], dtype, sparse, "no column with two levels")


@FORMS
@pytest.mark.parametrize("kind", [engine.FW_MI_NZ, engine.FW_NORM_TSS_BINNED], ids=["mi_nz", "tss_binned"])
def test_no_column_with_two_bins(kind, dtype, sparse):
    _refused(kind, [[1, 0], [0, 2], [0, 0]], dtype, sparse, "no column whose non-zero abundances fall into two bins")


def test_negative_count():
    _refused(engine.FW_FZ, [[1, -1], [2, 0]], np.int32, False, "negative count in column 1")


def test_nan_value():
    _refused(engine.FW_FZ, [[1, np.nan], [2, 0]], np.float64, False, "negative or non-finite (NaN, Inf) value in column 1")
