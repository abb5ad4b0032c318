"""Tables, jobs and the order-free reference shared by tests/test_fznz_edges_cpu.py and tests/test_gpu_fznz_edges.py: numpy only, no GPU
import.  Every generator is seeded by the sample count n, so the CPU module, the GPU module and a child process hold the same bytes.
All tables are Float32, column-major, zeros = absences (the clr_nz convention: a zero INSIDE a view is a value)."""
import functools

import numpy as np

N_OBS_MIN = 20
N_SMALL = (63, 64, 65, 127, 128, 129)   # last plane word partial / full
N_TREE, N_SEQ = 16384, 16385            # FZNZ_ROWS_LDS: the last n of the tree form, the first of the sequential form
N_LARGE = (16383, N_TREE, N_SEQ)
N_STAIR = 130                           # the small staircase: every view size of SIZES fits, and (n + 3) & ~3 != n
N_COND = {N_STAIR: 8, N_TREE: 6, N_SEQ: 6}
# rows of the views (0, 1 + j): 0 1 2 | 3 (zscale 0) | 4 | n_obs_min - 1, n_obs_min, n_obs_min + 1 | lanes of the 64-leaf tree with
# zero, one and two terms | 127 128 129 | every row.  The large tables hold 16 columns at most: nine views, six conditioning columns.
SIZES = {N_STAIR: (0, 1, 2, 3, 4, N_OBS_MIN - 1, N_OBS_MIN, N_OBS_MIN + 1, 63, 64, 65, 127, 128, 129, N_STAIR),
         N_TREE: (0, 3, N_OBS_MIN - 1, N_OBS_MIN, 64, 65, 129, 4100, N_TREE),
         N_SEQ: (0, 3, N_OBS_MIN - 1, N_OBS_MIN, 64, 65, 129, 4100, N_SEQ)}
ACC_SIZES = (0, 1, 2, 3, 6, 7, 14, 15)  # m = 2 3 4 | 5 (second tile row) | 8 9 | 16 17 (m_cap rounds up to a multiple of 16)


def _f32(x):
    x = np.asfortranarray(x.astype(np.float32))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def staircase(n):
    """Column 0 is non-zero in every row; column 1 + j in exactly SIZES[n][j] random rows, so the view (0, 1 + j) has exactly that many
    rows; behind them N_COND[n] conditioning columns, about 80 % filled.  A common factor keeps partial correlations away from 0."""
    sizes, nc = SIZES[n], N_COND[n]
    rng = np.random.default_rng(4000 + n)
    p = 1 + len(sizes) + nc
    f = rng.standard_normal((n, 1))
    sign = np.where(np.arange(p) % 3 == 2, -1.0, 1.0)
    x = (0.8 * f * sign + 0.6 * rng.standard_normal((n, p))).astype(np.float32)
    x[x == 0] = np.float32(0.25)
    for j, s in enumerate(sizes):
        keep = np.zeros(n, dtype=bool)
        keep[rng.choice(n, size=s, replace=False)] = True
        x[~keep, 1 + j] = 0.0
    first = 1 + len(sizes)
    x[:, first:] = np.where(rng.random((n, nc)) < 0.8, x[:, first:], np.float32(0.0))
    return _f32(x)


def stair_cond(n):
    """ids of the conditioning columns of staircase(n)"""
    first = 1 + len(SIZES[n])
    return list(range(first, first + N_COND[n]))


def stair_tests(n):
    """Every view x k = 0 .. 3 as explicit tests (0, 1 + j | Zs); the conditioning columns rotate with j."""
    cond = stair_cond(n)
    X, Y, Zs = [], [], []
    for j in range(len(SIZES[n])):
        for k in range(4):
            X.append(0); Y.append(1 + j); Zs.append(tuple(cond[(j + i) % len(cond)] for i in range(k)))
    return X, Y, Zs


def stair_jobs(n):
    """test_subsets jobs (0, 1 + j, accepted) for every view and every |accepted| of ACC_SIZES the table has the columns for: the
    conditioning columns first (rotated with j), then the other view columns (all-zero or constant inside most views: the NaN -> 0 of
    the matrix path, the NaN stop of the no-matrix path)."""
    cond = stair_cond(n)
    p = staircase(n).shape[1]
    T, C, A = [], [], []
    for j in range(len(SIZES[n])):
        pool = [cond[(j + i) % len(cond)] for i in range(len(cond))] + [v for v in range(p - 1, 0, -1) if v != 1 + j and v not in cond]
        for a in ACC_SIZES:
            if a <= len(pool):
                T.append(0); C.append(1 + j); A.append(pool[:a])
    return T, C, A


# chain: (a, fill) per n.  Zeros inside a view are values, so a conditioning column explains its neighbours only where it is present:
# the residual partial correlation of (j - 1, j + 1) given j is about a^2 (1 - fill) / (1 - a^2 fill), which 13 000 common rows detect
# unless the coupling is weak or the fill high.  Chosen on the oracle alone (tests/test_fznz_edges_cpu.py asserts the shares).
CHAIN = {63: (0.85, 0.9), 64: (0.85, 0.9), 65: (0.85, 0.9), 127: (0.85, 0.9), 128: (0.85, 0.9), 129: (0.85, 0.9),
         16383: (0.6, 0.98), 16384: (0.6, 0.98), 16385: (0.6, 0.98)}


@functools.lru_cache(maxsize=None)
def chain(n, p=16, a=None, fill=None):
    """Column j = a * column j - 1 + sqrt(1 - a^2) * noise (unit variance, mean 0), present with probability `fill`: conditioning on
    the column between two others really removes their edge."""
    if a is None:
        a, fill = CHAIN[n]
    rng = np.random.default_rng(5000 + n)
    x = np.empty((n, p))
    x[:, 0] = rng.standard_normal(n)
    for j in range(1, p):
        x[:, j] = a * x[:, j - 1] + np.sqrt(1.0 - a * a) * rng.standard_normal(n)
    x = x.astype(np.float32)
    x[x == 0] = np.float32(0.25)
    return _f32(np.where(rng.random((n, p)) < fill, x, np.float32(0.0)))


@functools.lru_cache(maxsize=None)
def wide(n=130, p=520):
    """A common factor plus noise, 85 % filled: room for accepted lists of 512 and 513 variables."""
    rng = np.random.default_rng(6000 + n)
    f = rng.standard_normal((n, 1))
    sign = np.where(rng.random(p) < 0.5, -1.0, 1.0)
    x = (0.9 * f * sign + 0.55 * rng.standard_normal((n, p))).astype(np.float32)
    x[x == 0] = np.float32(0.25)
    x = np.where(rng.random((n, p)) < 0.85, x, np.float32(0.0))
    x[:, :2] = np.where(x[:, :2] == 0, np.float32(0.5), x[:, :2])  # the pair of the long-list jobs: a view of every row
    return _f32(x)


def wide_jobs():
    """-> (long batch, small batch) of (T, candidate, accepted): the long batch holds |accepted| = 62, 63, 64 (m = 64, 65, 66:
    FZNZ_DEV_SMALL) and 512, 513 (FW_TAB_A: table kernel and in-lane kernel on job-local matrices) next to short lists; the small
    batch only short lists, so m_cap differs between the two launches."""
    p = wide().shape[1]
    rng = np.random.default_rng(6001)
    T, C, A = [], [], []
    for a in (62, 63, 64, 512, 513, 3, 14):
        others = rng.permutation(np.arange(2, p))
        T.append(0); C.append(1); A.append([int(v) for v in others[:a]])
    for a in (63, 512, 513):  # an ordinary pair as well: a view of ~ 0.72 n rows
        t, c = int(rng.integers(2, p)), int(rng.integers(2, p - 1))
        c += c >= t
        others = [int(v) for v in rng.permutation(p) if v not in (t, c)]
        T.append(t); C.append(c); A.append(others[:a])
    Ts, Cs, As = [], [], []
    for a in (1, 2, 3, 6, 7, 10):
        v = [int(u) for u in rng.choice(p, size=a + 2, replace=False)]
        Ts.append(v[0]); Cs.append(v[1]); As.append(v[2:])
    return (T, C, A), (Ts, Cs, As)


@functools.lru_cache(maxsize=None)
def hub(n=130, p=110):
    """Variable 0 is the hub, every other one a noisy copy of it, independent of each other given the hub: the hub's accepted list grows
    past 62 entries (jobs of more than FZNZ_DEV_SMALL = 64 variables).  Variables 100 .. 103 are means of two copies each, so rejections
    happen against long lists.  8 % of the ordinary cells are absent."""
    rng = np.random.default_rng(7000 + n)
    h = rng.standard_normal(n)
    x = 2.0 + 0.9 * h[:, None] + 0.55 * rng.standard_normal((n, p))
    x[:, 0] = 2.0 + h
    for y, (a, b) in ((100, (1, 2)), (101, (3, 4)), (102, (5, 6)), (103, (7, 8))):
        x[:, y] = 0.5 * (x[:, a] + x[:, b]) + 0.1 * rng.standard_normal(n)
    present = rng.random((n, p)) < 0.92
    present[:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 100, 101, 102, 103]] = True
    return _f32(np.where(present, x, 0.0))


@functools.lru_cache(maxsize=None)
def nan_directed(n=65, p=12):
    """-> (table, T, candidate, z, others): z is present elsewhere but absent in every row of the (T, candidate) view, i.e. constant
    inside it -- a zero sum of squares, 0 / 0, which the matrix path turns into a correlation of 0."""
    rng = np.random.default_rng(8000 + n)
    f = rng.standard_normal((n, 1))
    x = (0.8 * f + 0.6 * rng.standard_normal((n, p))).astype(np.float32)
    x[x == 0] = np.float32(0.25)
    x = np.where(rng.random((n, p)) < 0.85, x, np.float32(0.0))
    T, Cn, z = 0, 1, 2
    both = (x[:, T] != 0) & (x[:, Cn] != 0)
    x[both, z] = 0.0
    assert both.sum() >= 2 * N_OBS_MIN and (x[:, z] != 0).sum() >= 3
    return _f32(x), T, Cn, z, [3, 4, 5, 6]


def to_triple(dense):
    """CSC triple of a dense Float32 matrix (colptr int64, rowval int32, nzval float32), an entry per value != 0"""
    keep = dense != 0
    colptr = np.concatenate([[0], np.cumsum(keep.sum(axis=0))]).astype(np.int64)
    rows = np.concatenate([np.nonzero(keep[:, c])[0] for c in range(dense.shape[1])]).astype(np.int32)
    vals = np.concatenate([dense[keep[:, c], c] for c in range(dense.shape[1])]).astype(np.float32)
    return colptr, rows, vals


def view_rows(data, x, y):
    return np.nonzero((data[:, x] != 0) & (data[:, y] != 0))[0]


def pcor_longdouble(data, x, y, zs):
    """Order-free reference of one fz_nz test without a matrix: the rows where x and y are both non-zero, the columns centred, their
    Gram matrix, the recursion of StatsBase.partialcor (condition on the last variable, then the one before, ...), clamp -- all in
    numpy.longdouble, sums by numpy's pairwise summation.  -> (statistic as a Python float, rows of the view)"""
    rows = view_rows(data, x, y)
    if len(rows) == 0:
        return float("nan"), 0
    v = data[np.ix_(rows, [x, y] + list(zs))].astype(np.longdouble)
    v = v - v.mean(axis=0)
    m = v.shape[1]
    g = np.array([[(v[:, a] * v[:, b]).sum() for b in range(m)] for a in range(m)], dtype=np.longdouble)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.sqrt(np.diag(g))
        r = g / np.outer(d, d)
        for t in range(m - 1, 1, -1):
            for a in range(t):
                for b in range(a + 1, t):
                    r[a, b] = r[b, a] = (r[a, b] - r[a, t] * r[b, t]) / (np.sqrt(1 - r[a, t] ** 2) * np.sqrt(1 - r[b, t] ** 2))
    out = r[0, 1]
    out = min(max(out, np.longdouble(-1)), np.longdouble(1)) if not np.isnan(out) else out
    return float(out), len(rows)


# ---- the oracle's side: one context per table and form, shared by both test modules, never written to ----

TABLES = {"staircase": staircase, "chain": chain, "wide": lambda n: wide(n), "hub": lambda n: hub(n), "nan": lambda n: nan_directed(n)[0]}


@functools.lru_cache(maxsize=None)
def oracle_of(name, n, stream=False, p=None):
    """The oracle on a table (Float32 values, Float64 arithmetic, as on the device); stream: conditional tests without a matrix."""
    from oracle import oracle as O
    data = chain(n, p) if p is not None else TABLES[name](n)
    orc = O.Oracle("fz_nz", data=data.astype(np.float64))
    if stream:
        orc.set_fz_nz_stream(True)
    return orc


def full_count(a, max_k=3):
    """number of subsets of sizes 1 .. max_k of a list of a variables"""
    out, c = 0, 1
    for j in range(1, max_k + 1):
        c = c * (a - j + 1) // j
        out += c
    return out
