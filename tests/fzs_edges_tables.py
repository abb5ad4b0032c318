"""Tables, jobs and the order-free reference shared by tests/test_fzs_edges_cpu.py and tests/test_gpu_fzs_edges.py: numpy only, no GPU
import.  Every generator is deterministic in its arguments, so the CPU module and the GPU module hold the same bytes.  All tables are
Float32, column-major.  DESIGN.md section 4.7 lists the switches of the fzs_* kernels (fw_fzs.hip) these shapes are chosen for."""
import functools

import numpy as np

N_OBS_MIN = 20
# fzs_hold_xy (n % 4 == 0 && n <= 2048), the 256-sample rows of the float4 loops, the 64-sample steps of the generic loops
N_ALL = (60, 63, 64, 65, 68, 252, 253, 254, 255, 256, 257, 260, 2044, 2048, 2049, 2050, 2051, 2052)
N_NET = (255, 256, 2048, 2049)
N_NET_NO_MATRIX = (255, 2049)
N_LISTS = (64, 257)
N_OFFSET = (255, 2000)
RATIOS = (30, 1000, 30000)
P_SINGLE, P_NET, P_LISTS = 24, 40, 130
LIST_LENGTHS = (1, 2, 3, 6, 10, 14, 77, 78, 79, 80)  # m = a + 2: 3 4 5 | 8 | 12 | 16 | 79 80 81 82 (multiples of 4, the LDS limit of 80)
LIST_CAP = 3002           # max_tests of the list-length batch: the last test has rank 3001, the second of its group of four
CAPS_IN_GROUP = (3001, 3002, 3003)
LIST_ALPHA = 0.9999
CHAIN = 6                 # columns per chain
CONST_VALUE = 1.5


def _f32(x):
    x = np.asfortranarray(x.astype(np.float32))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _base(n, p, seed):
    """Float64, unit variance, mean 0: chains of CHAIN columns, column j = 0.7 * column j - 1 + noise, so conditioning on the column
    between two others removes their edge at every n; the head of a chain loads 0.6 on one of three shared factors, so the chains
    are neighbours of each other at level 0 as well.  Population |r| <= 0.7."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((n, 3))
    x = np.empty((n, p))
    for j in range(p):
        e = rng.standard_normal(n)
        x[:, j] = 0.6 * f[:, (j // CHAIN) % 3] + 0.8 * e if j % CHAIN == 0 else 0.7 * x[:, j - 1] + np.sqrt(0.51) * e
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def centred(n, p, seed=0):
    return _f32(_base(n, p, 9000 + seed))


@functools.lru_cache(maxsize=None)
def offset(n, p, seed, ratio):
    """The columns of `centred` plus ratio * sigma each; the cast to Float32 IS the table (at ratio 30 000 the values are multiples of
    2^-9: every value is exactly what both sides read)."""
    b = _base(n, p, 9000 + seed)
    return _f32(b + ratio * b.std(axis=0))


CONST_COL, TWIN_COL, TWIN_SRC = 22, 23, 3


def with_constant(table, col=CONST_COL, value=CONST_VALUE):
    x = np.array(table, order="F")
    x[:, col] = np.float32(value)
    return _f32(x)


def with_twin(table, col=TWIN_COL, src=TWIN_SRC):
    """column `col` becomes an exact copy of column `src`: another variable with the same values (r = 1 from the sums, no id rule)"""
    x = np.array(table, order="F")
    x[:, col] = x[:, src]
    return _f32(x)


@functools.lru_cache(maxsize=None)
def degenerate(n):
    return with_twin(with_constant(centred(n, P_SINGLE)))


# ---- jobs ----

@functools.lru_cache(maxsize=None)
def single_tests(p=P_SINGLE, kmax=5, count=47, seed=1):
    """-> (X, Y, Zs): k = 0 .. kmax mixed, every k at least twice; count % 4 == 3, so the last workgroup of the batch kernel holds
    three tests and the last index is no multiple of 4"""
    assert count % 4 == 3
    rng = np.random.default_rng(seed)
    X, Y, Zs = [], [], []
    for i in range(count):
        k = i % (kmax + 1) if i < 2 * (kmax + 1) else int(rng.integers(0, kmax + 1))
        v = rng.choice(p, size=k + 2, replace=False)
        X.append(int(v[0])); Y.append(int(v[1])); Zs.append(tuple(int(t) for t in v[2:]))
    return X, Y, Zs


def nine_jobs(p=P_SINGLE):
    """test_subsets jobs with 9 accepted variables.  For every chain c: (c+1, c+3 | ... c+2 ...) with the column between the two at
    position 0, 4 or 8 of the list (the job stops once a subset holds it: at rank 0, inside the first run, late in it), and
    (c+1, c+2 | nine columns of the other chains) -- neighbours in a chain stay dependent whatever else is conditioned on, so the
    enumeration runs to its end."""
    T, C, A = [], [], []
    for ci, c in enumerate(range(0, p, CHAIN)):
        others = [v for v in range(p) if v // CHAIN != c // CHAIN]
        rot = others[3 * ci:] + others[:3 * ci]
        lst = rot[:8]
        lst.insert((0, 4, 8)[ci % 3], c + 2)
        T.append(c + 1); C.append(c + 3); A.append(lst)
        T.append(c + 1); C.append(c + 2); A.append(rot[:9])
    return T, C, A


def list_jobs(p=P_LISTS):
    """(0, 1 | a columns from the other chains) and an ordinary pair for every a of LIST_LENGTHS"""
    rng = np.random.default_rng(77)
    T, C, A = [], [], []
    for a in LIST_LENGTHS:
        others = [int(v) for v in rng.permutation(np.arange(CHAIN, p))]
        T.append(0); C.append(1); A.append(others[:a])
        v = [int(u) for u in rng.choice(p, size=a + 2, replace=False)]
        T.append(v[0]); C.append(v[1]); A.append(v[2:])
    return T, C, A


def offset_tests(p=P_SINGLE):
    """explicit tests with k = 1 .. 3 inside and across chains, 27 of them"""
    rng = np.random.default_rng(3)
    X, Y, Zs = [], [], []
    for i in range(27):
        k = 1 + i % 3
        c = CHAIN * (i % (p // CHAIN))
        v = [c + 1, c + 2, c + 3, c, c + 4] if i < 12 else [int(t) for t in rng.choice(p, size=k + 2, replace=False)]
        X.append(v[0]); Y.append(v[1]); Zs.append(tuple(v[2:2 + k]))
    return X, Y, Zs


# the degenerate explicit tests: (name, X, Y, Zs, kind).  kind "value": the statistic is defined, compared at the usual tolerance;
# "0/0": some step of the recursion is 0 / 0 in exact arithmetic -- NaN-ness, p and suff_power are compared, not the digits.
DEGENERATE_TESTS = (
    ("constant X", CONST_COL, 1, (2,), "0/0"),
    ("constant X, k = 2", CONST_COL, 1, (2, 7), "0/0"),
    ("constant Z", 0, 1, (CONST_COL,), "0/0"),
    ("constant Z first of two", 0, 1, (CONST_COL, 2), "0/0"),
    ("constant Z last of two", 0, 1, (2, CONST_COL), "0/0"),
    ("twin of an outsider as Z", 0, 1, (TWIN_COL,), "value"),
    ("twin of an outsider as Z, k = 3", 0, 1, (8, TWIN_COL, 14), "value"),
    ("twin of X as Z", TWIN_SRC, 4, (TWIN_COL,), "0/0"),
    ("a column and its twin both in Z", 0, 1, (TWIN_SRC, TWIN_COL), "0/0"),
    ("the same variable twice in Z", 0, 1, (2, 2), "0/0"),
    ("the same variable twice in Z, k = 3", 0, 1, (7, 2, 2), "0/0"),
    ("X again in Z", 2, 5, (2,), "0/0"),
)

# test_subsets jobs on degenerate(n): (name, T, candidate, accepted)
DEGENERATE_JOBS = (
    ("a variable twice in the list", 1, 2, (8, 13, 8, 19, 14)),
    ("a variable twice, first and last", 7, 8, (13, 0, 19, 13)),
    ("the constant column in the list", 1, 2, (8, 13, CONST_COL, 19)),
    ("the constant column as candidate", 1, CONST_COL, (8, 13, 19)),
    ("a column and its twin in the list", 7, 8, (13, TWIN_SRC, 19, TWIN_COL)),
    ("the twin of an outsider in the list", 7, 8, (13, TWIN_COL, 19)),
)


def full_count(a, max_k=3):
    """number of subsets of sizes 1 .. max_k of a list of a variables"""
    out, c = 0, 1
    for j in range(1, max_k + 1):
        c = c * (a - j + 1) // j
        out += c
    return out


# ---- the order-free reference ----

def pcor_ld(data, x, y, zs):
    """One conditional test in numpy.longdouble: fully centred sums (numpy's pairwise summation), then the (k + 2) x (k + 2)
    correlation matrix conditioned on Z_k, ..., Z_1 as fwo_pcor documents (StatsBase.partialcor unrolled), clamp.  -> Python float"""
    v = np.asarray(data)[:, [x, y] + list(zs)].astype(np.longdouble)
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
    if not np.isnan(out):
        out = min(max(out, np.longdouble(-1)), np.longdouble(1))
    return float(out)


# ---- the oracle's side: one context per table, shared by both test modules, never written to ----

@functools.lru_cache(maxsize=None)
def oracle_of(kind, n, p, ratio=0, cor="oracle"):
    """The oracle on a table with conditional tests through pcor (set_fz_data).  kind: "centred" | "offset" | "degenerate".
    cor = "oracle": its own Float32 Pearson matrix (level 0, univariate tests); "eye": none is needed (conditional tests only)."""
    from oracle import oracle as O
    data = table_of(kind, n, p, ratio)
    d64 = data.astype(np.float64)
    cm = O.cor(d64, "f32") if cor == "oracle" else np.eye(p, dtype=np.float32)
    orc = O.Oracle("fz", cor_mat=cm, n_obs=n)
    orc.set_fz_data(d64)
    return orc


def table_of(kind, n, p, ratio=0):
    if kind == "centred":
        return centred(n, p)
    if kind == "offset":
        return offset(n, p, 0, ratio)
    assert kind == "degenerate" and p == P_SINGLE
    return degenerate(n)
