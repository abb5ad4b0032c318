"""Tables and helpers shared by tests/test_norm_mode_cpu.py and tests/test_gpu_norm_mode.py: a helper module, not a test."""
import numpy as np
import scipy.sparse as sp

from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd.engine import CSC
from tests.api_trace import _scatter
from tests.util import GOLDEN

TSS_MODES = ("tss", "tss-nonzero-binned")
ALIASES = {"clr-adapt": "fz", "clr-nonzero": "fz_nz", "clr-nonzero-binned": "mi_nz", "pres-abs": "mi"}


def hmp():
    """the bundled 351 x 50 count table"""
    return np.loadtxt(GOLDEN + "/HMP_SRA_gut_small.tsv", delimiter="\t", skiprows=1, usecols=range(1, 51)).astype(np.int64)


def fixture(mode):
    """the reference's expected output for a TSS mode: Float32 values as printed / Int32 levels"""
    if mode == "tss":
        return np.loadtxt(GOLDEN + "/tss.tsv").astype(np.float32)
    return np.loadtxt(GOLDEN + "/tss_nonzero_binned.tsv").astype(np.int32)


def bits(a):
    """a Float32 / Float64 array as integers: equality of these is equality to the bit (-0.0 and 0.0 differ, NaNs compare)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def dense(m):
    """a normalised table as a dense array (a stored 0.0f of a sparse one becomes a plain zero)"""
    return np.asarray(m.toarray()) if sp.issparse(m) else np.asarray(m)


def host_stand_in(counts, test_name, device=0, **kw):
    """fw.api.normalize_counts / normalize_abundances on the host, as tests/api_trace._host_stand_in does it, for calls that carry a
    norm: preprocess.normalize on the table (a sparse one scattered first), a sparse table handed back in CSC form with one entry
    per present value, as the device front-end returns it."""
    if not isinstance(counts, CSC):
        return pre.normalize(counts, test_name, **kw)
    table = _scatter(*counts)
    data, row_mask, col_mask = pre.normalize(table, test_name, **kw)
    present = table[row_mask][:, col_mask] != 0
    cols, rows = np.nonzero(present.T)
    out = sp.csc_matrix(data.shape, dtype=data.dtype)
    out.indptr = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=data.shape[1])))).astype(np.int32)
    out.indices, out.data = rows.astype(np.int32), data[rows, cols]
    return out, row_mask, col_mask


def f32_sum_left_to_right(row):
    s = np.float32(0)
    for v in np.asarray(row, dtype=np.float32):
        s = np.float32(s + v)
    return s


def edge_table(n=257, p=130):
    """Counts for the device tests: n crosses a 64-lane and a 256-thread boundary, p is more than the 64 column chunks of the clr
    kernels.  Column 5 is constant and non-zero (it must not enter a row sum), samples 9 and 200 are empty, samples 20 and 21 hold
    1 of 3 and 2 of 6 in column 0 (equal quotients: a tie), and sample 30 holds 2^24 in its first kept column followed by ones, so
    that its Float32 sum depends on the order of the additions."""
    i, j = np.indices((n, p))
    x = (5 * i * i + 3 * j * j + 7 * i * j + i + 11 * j) % 23
    x[x < 13] = 0  # more than half of the cells are zeros
    x[20], x[21] = 0, 0
    x[20, [0, 1]], x[21, [0, 1]] = (1, 2), (2, 4)
    x[30] = 1
    x[30, 0] = 2 ** 24
    x[[9, 200]] = 0  # (empty over the kept columns: the constant column below is all they hold)
    x[:, 5] = 4
    return x.astype(np.int64)
