"""The bytes the device normalisation front-end returns: a helper module, not a test (tests/test_gpu_norm_bytes.py compares what it
returns with tests/golden/norm_bytes.json).  It uses engine.normalize_counts / normalize_abundances only, so the same file runs on
any commit.  The golden file was recorded ON THE PARENT COMMIT of the change that split the host half of csrc/fw_norm.hip into
stages, on an MI355X, before any of that refactoring (`python -m tests.norm_bytes --write` in a checkout of the parent with this
file copied in) -- never on the code under test.  A later change that moves bytes on purpose records it again on ITS parent.

A case is one call.  Its digest is the SHA-256 over the output -- a dense array as its dtype, shape and column-major bytes, a sparse
one as data / indices / indptr -- followed by the sample mask and the column mask.  Every output is Int32, or Float32 from Float64
expressions whose libm calls run on the device: the digest ties the golden to the device library, which is what it is there to pin.

The tables come from fixed seeds:
  t70     70 x 67 counts: 65 kept columns (more than the 64 column chunks of the row statistics, per = 2: the last chunk holds one
          column), 70 rows (no multiple of 64); two all-zero columns, a sample without reads, a column full among the samples with
          reads (dropped by "mi"), a column with one non-zero (dropped by "mi_nz" and "tss-nonzero-binned": one bin), the sample of
          maximal depth three times (ties of the anchor and of the ranks).  Int32, the same as Float64, and as relative abundances.
  t16400  16 400 x 8, column 0 full: more than 16 384 sort keys per column, dense (kept samples) and CSC (longest column) -- the keys
          go to device memory.  "mi_nz" and "tss-nonzero-binned".
  t2100   2 100 x 6, every column full, CSC only: 2 049 .. 16 384 keys, the 1 024-thread shape of the CSC binned kernel.
  t80000  4 x 80 000 with values 0..3, dense only, "fz" and "mi": more than 65 535 output columns, so the output kernels loop beyond
          the limit on grid.y.  Half of the cells are zero (the other values equally likely): under a uniform draw "mi" would keep
          about 54 400 columns -- those with a zero and a non-zero among four samples -- and never visit the loop."""
import functools
import hashlib
import json
import os
import sys

import numpy as np
import scipy.sparse as sp

from flashweave_jl_amd import engine

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_bytes.json")
KINDS = {"fz": ("fz", None), "fz_nz": ("fz_nz", None), "mi": ("mi", None), "mi_nz": ("mi_nz", None), "tss": ("fz", "tss"),
         "tss_binned": ("mi_nz", "tss-nonzero-binned")}
BINNED = ("mi_nz", "tss_binned")


@functools.lru_cache(maxsize=None)
def table(name):
    """the integer tables, as int64"""
    if name == "t70":
        x = np.random.default_rng(70).integers(0, 9, size=(70, 67))
        x[x < 4] = 0  # about 45 % zeros
        x[3] = 3 * x[3] + 1  # the deepest sample ...
        x[10], x[41] = x[3], x[3]  # ... three times
        x[:, 5], x[:, 40] = 0, 0  # constant
        x[:, 12] = 1 + np.arange(70) % 5  # full
        x[:, 30] = 0
        x[17, 30] = 6  # one non-zero
        x[25] = 0  # no reads
        return x
    if name == "t16400":
        x = np.random.default_rng(16400).integers(0, 6, size=(16400, 8))
        x[:, 0] += 1
        return x
    if name == "t2100":
        return np.random.default_rng(2100).integers(1, 50, size=(2100, 6))
    if name == "t80000":
        return np.random.default_rng(80000).choice(4, size=(4, 80000), p=[0.5, 1 / 6, 1 / 6, 1 / 6])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def relative():
    """t70 as relative abundances (the sample without reads stays empty)"""
    x = table("t70").astype(np.float64)
    return x / np.maximum(x.sum(axis=1, keepdims=True), 1.0)


CASES = {}  # name -> (table, value type, form, kind)


def _cases(tab, values, forms, kinds):
    for v in values:
        for form in forms:
            for k in kinds:
                CASES["%s_%s_%s_%s" % (tab, v, form, k)] = (tab, v, form, k)


_cases("t70", ("i32", "f64", "rel"), ("dense", "csc"), KINDS)
_cases("t16400", ("i32", "f64"), ("dense", "csc"), BINNED)
_cases("t2100", ("i32", "f64"), ("csc",), BINNED)
_cases("t80000", ("i32", "f64"), ("dense",), ("fz", "mi"))


def run_case(name):
    """One case -> (digest, shape of the output)."""
    tab, values, form, kind = CASES[name]
    x = relative() if values == "rel" else table(tab)
    front_end = engine.normalize_counts if values == "i32" else engine.normalize_abundances
    x = x.astype(np.int32 if values == "i32" else np.float64)
    test_name, norm = KINDS[kind]
    out, row_mask, col_mask = front_end(sp.csc_matrix(x) if form == "csc" else x, test_name, **({} if norm is None else {"norm": norm}))
    h = hashlib.sha256()
    if sp.issparse(out):
        parts = [np.asarray(out.data), np.asarray(out.indices), np.asarray(out.indptr)]
    else:
        parts = [np.asfortranarray(out)]
    for a in parts + [np.asarray(row_mask), np.asarray(col_mask)]:
        h.update(("%s%r" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes(order="F"))
    return h.hexdigest(), tuple(int(v) for v in out.shape)


def run_all():
    return {name: run_case(name)[0] for name in CASES}


def load_golden():
    with open(GOLDEN_FILE) as fh:
        return json.load(fh)


if __name__ == "__main__":
    digests = run_all()
    if "--write" in sys.argv[1:]:
        with open(GOLDEN_FILE, "w") as fh:
            json.dump(digests, fh, indent=0, sort_keys=True)
            fh.write("\n")
        print("wrote %d cases -> %s" % (len(digests), GOLDEN_FILE))
    else:
        for k, v in digests.items():
            print(k, v)
