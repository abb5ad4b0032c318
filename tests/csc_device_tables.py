"""Tables of the sparse-CSC device-tensor tests (tests/test_gpu_csc_device_tables.py, tests/test_csc_device_tables_cpu.py): plain
numpy / scipy, so that both files build the same inputs.  Every table comes as a canonical scipy.sparse.csc_matrix -- rows ascending in
every column, no duplicates, no stored zeros unless a test asks for them -- which is what torch.sparse_csc_tensor is built over."""
import numpy as np
import scipy.sparse as sp

N_GRID = (63, 64, 65, 130)  # plane-word edges and a ragged last word
P_GRID = (5, 129)  # within and across one level-0 tile of 128 variables
TOPS = (1, 2, 3, 61)  # the largest level: two planes' worth, the switch to the generic form, the top of the range


def discrete_dense(n, p, top):
    """levels 0 .. min(top, 2) that follow three hidden columns (so that level 0 and the network are not empty), as a dense Int32
    table with
      column 0   entries in rows 0, 63, 64 and n - 1 (those that exist)
      column 1   empty
      column 2   all n entries: no implicit zero level, and more than 64 entries at n = 130
      column 3   entries only in the last plane word (rows >= 64 * ((n - 1) // 64)), which is ragged unless n is a multiple of 64
    top 3 / 61: that value once, in the last row of the last column -- the switch to the generic form, the top of the range"""
    rng = np.random.default_rng(1000 * n + 10 * p + top)
    hi = min(top, 2)
    hidden = rng.integers(0, hi + 1, size=(n, 3))
    x = np.where(rng.random((n, p)) < 0.75, hidden[:, np.arange(p) % 3], rng.integers(0, hi + 1, size=(n, p))).astype(np.int32)
    for r in (0, 63, 64, n - 1):
        if r < n:
            x[r, 0] = max(x[r, 0], 1)
    x[:, 1] = 0
    x[:, 2] = 1 + np.arange(n) % hi
    last = 64 * ((n - 1) // 64)
    x[:last, 3] = 0
    x[last:, 3] = 1 + np.arange(n - last) % hi
    if top > 2:
        x[n - 1, p - 1] = top
    return x


def discrete_csc(n, p, top):
    m = sp.csc_matrix(discrete_dense(n, p, top))
    m.sort_indices()
    assert m.data.min() >= 1 and m.data.max() == top and m.has_canonical_format
    return m


def fznz_csc(n, p, dtype):
    """Float values that follow three hidden columns, 40 % absences, in the column layout of discrete_dense; three STORED entries
    that are absences to the engine: a 0.0, a -0.0 and a 1e-60 (which rounds to 0.0f; with dtype float32 it is a 0.0 already)"""
    rng = np.random.default_rng(2000 * n + p)
    hidden = rng.standard_normal((n, 3))
    x = hidden[:, np.arange(p) % 3] + 0.7 * rng.standard_normal((n, p))
    x[rng.random((n, p)) < 0.4] = 0.0
    for r in (0, 63, 64, n - 1):
        if r < n:
            x[r, 0] = 1.5 + r
    x[:, 1] = 0.0
    x[:, 2] = 1.0 + rng.random(n)
    last = 64 * ((n - 1) // 64)
    x[:last, 3] = 0.0
    x[last:, 3] = 2.0 + rng.random(n - last)
    x[2, 0], x[5, p - 1], x[7, p - 1] = 7.0, 7.0, 7.0  # (stored below as the three zeros)
    m = sp.csc_matrix(x.astype(dtype))
    m.sort_indices()
    stored = {(2, 0): 0.0, (5, p - 1): -0.0, (7, p - 1): 1e-60}
    for (r, c), v in stored.items():
        k = m.indptr[c] + int(np.searchsorted(m.indices[m.indptr[c]:m.indptr[c + 1]], r))
        assert m.indices[k] == r
        m.data[k] = v
    assert np.signbit(m.data[m.data == 0]).any() and (np.float32(m.data) == 0).sum() == 3
    return m


def count_csc():
    """200 x 40 synthetic counts (flashweave_jl_amd.synth) with sample 17 emptied (zero reads) and column 5 made constant -- all zero,
    the one constant an empty sample leaves room for: both masks drop something"""
    from flashweave_jl_amd import synth
    x = np.array(synth.generate(40, 200, seed=5))
    x[17, :] = 0
    x[:, 5] = 0
    m = sp.csc_matrix(x)
    m.sort_indices()
    return m


class FakeSparseCscTensor:
    """Stands in for a sparse CSC tensor in GPU memory where no GPU is: tests/test_csc_device_tables_cpu.py makes the predicates of
    flashweave_jl_amd accept it, so that the refusals -- which come before any library call -- can be read on a host without a device"""

    class _Dev:
        type, index = "cuda", 0

        def __str__(self):
            return "cuda:0"

    def __init__(self, m, layout, dtype=None):
        import torch
        self._m, self.layout, self.device = m, layout, self._Dev()
        self.shape = tuple(m.shape)
        self.dtype = dtype or torch.from_numpy(m.data[:1]).dtype

    def dim(self):
        return len(self.shape)

    def values(self):
        import torch
        return torch.from_numpy(np.ascontiguousarray(self._m.data))
