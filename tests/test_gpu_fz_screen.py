"""The Float32 screen of the size-3 Fisher-z table kernel (fw_fz_core.h, fz_seg_body, `#if FW_FZ_SCREEN`) on the device, through the C ABI
of the shipped library, at its guard edges: constructed correlation matrices (Engine.set_cor_mat; neither the library nor the oracle needs
them positive definite) whose size-3 tests sit inside the guard windows d1 ~ 0.01, g ~ 0.02, Pb / Pc ~ dl, on plateaus of nearly or exactly
equal |stat|^2, in the underflow regime of p, next to NaN entries and on a max_tests cap -- compared with the oracle the way
tests/test_gpu_fz.py::_check_subsets does (status, num_tests, Zs, stat exact; pval, frac to 1e-12).

WHEN THE SCREEN RUNS AT ALL.  The fast loop needs a chunk that lies wholly inside the size-3 enumeration (`ilv`: cend <= C(a, 3)), and the
screen needs a bound to compare with, i.e. a lane that has ALREADY taken an exact test in the same segment: runs of R >= 2 ranks per lane.
A chunk is min(segment, 256 R) ranks, R = ceil(len / 256) <= 64; the host (fwi_pool_add / fwi_pool_launch, fw_pool.cpp) cuts a job's window
(first 256 ranks, 16 384 from 64 accepted variables on; everything that is left afterwards in these small launches) into segments of
    seglen = clamp(ceil256(ranks of the launch / 3072), 256, 8192),
so (a) alone in a launch, a job has segments of 256 ranks whatever its length: R = 1, one test per lane, and the screen only ever meets a
bound another wavefront happened to publish first; (b) in ONE segment a job needs |accepted| >= 48 (C(48, 3) = 17 296 > 16 384) for a
full-length chunk inside size 3, in the pool's segments of at most 8 192 ranks |accepted| >= 38; (c) what makes R >= 2 is the LAUNCH: more
than 3072 * 256 = 786 432 ranks in flight.  Every batch here therefore holds dozens of all-significant jobs of 48, 64 and 100 accepted
variables (48 is the one-segment length, 64 switches the first window to 16 384), and _plan() -- the host's rule restated -- asserts
R >= 2 on segments inside size 3 before anything is uploaded.  The directed cases of tests/test_gpu_fz.py (lists of 9-30, a few dozen
jobs) run R = 1 or the general form: they are NOT screen coverage.

COVERAGE is asserted through tests/screen_model.py (a numpy restatement of the screen): at least 1 000 size-3 tests of each batch pass every
guard inside the family's window.  The model chooses inputs and counts; expected values are the oracle's.

What a wrong screen looks like: a skipped test that was the maximum-p test of its job -> wrong Zs / stat, nothing else.  The `ties` family is
built from operand tuples of screen_model.directed_search (tests/golden/screen_tuples.json) on which a dl of one twentieth fails, see
profiles/screen_directed.txt.
"""
import json
import math
import os

import numpy as np
import pytest

import flashweave_jl_amd as fw
from oracle import oracle as O
from tests import screen_model as M
from tests.pool_plan import _job_ranks, _plan
from tests.util import GOLDEN, rel

pytestmark = pytest.mark.gpu

f32, f64 = np.float32, np.float64
N_OBS = 300  # sure range of |stat| at alpha = 0.01: about (0.149, 0.973)


# ---- the host's segmenting: tests/pool_plan.py restates fw_pool_host.h / fw_pool.cpp (tests/test_pool_host_cpu.py holds the two together) ----
def _screen_segments(alens, max_tests=10_000_000):
    """Segments of the batch that lie wholly inside the size-3 enumeration with runs of R >= 2 ranks per lane -> (count, smallest R, largest R)."""
    n, rs = 0, []
    for seglen, wins in _plan(alens, max_tests):
        for i, lo, hi in wins:
            c3 = math.comb(alens[i], 3)
            for s in range(lo, hi, seglen):
                e = min(hi, s + seglen)
                R = min(-(-(e - s) // 256), 64)
                if e <= c3 and R >= 2:
                    n += 1
                    rs.append(R)
    return n, (min(rs) if rs else 0), (max(rs) if rs else 0)


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def _same(g, e):
    return g == e or (np.isnan(g) and np.isnan(e))


def _check_batch(cm, n_obs, X, Y, A, max_tests=10_000_000):
    """test_subsets_batch on the uploaded matrix against Oracle.test_subsets (tests/test_gpu_fz.py::_check_subsets); identical jobs are
    asked of the oracle once."""
    p = cm.shape[0]
    eng = fw.Engine("fz", n_obs, p, max_k=3, max_tests=max_tests)
    eng.set_cor_mat(cm)
    got = eng.test_subsets_batch(X, Y, A)
    eng.close()
    orc = O.Oracle("fz", cor_mat=cm, n_obs=n_obs)
    memo = {}
    statuses = []
    for x, y, a, g in zip(X, Y, A, got):
        key = (x, y, tuple(a))
        if key not in memo:
            memo[key] = orc.test_subsets(x, y, a, max_k=3, alpha=0.01, n_obs_min=20, max_tests=max_tests)
        e = memo[key]
        statuses.append(e["status"])
        assert g["status"] == e["status"], (x, y, len(a), g, e)
        assert g["num_tests"] == e["num_tests"], (x, y, len(a), g, e)
        if e["status"] == 0:
            assert np.isnan(g["stat"]) and np.isnan(g["pval"]) and g["df"] == -1
            continue
        assert g["Zs"] == e["Zs"], (x, y, len(a), g, e)
        assert _same(g["stat"], e["stat"]), (g, e)
        assert rel(g["pval"], e["pval"]) < 1e-12 or (np.isnan(g["pval"]) and np.isnan(e["pval"]))
        assert rel(g["frac"], e["frac"]) < 1e-12
    orc.close()
    return statuses, memo


def _coverage(cm, X, Y, A, window, sample=6):
    """Size-3 tests of (a sample of) the batch that pass every guard of the screen inside the family's window, by the model."""
    n = 0
    step = max(1, len(A) // sample)
    for x, y, a in list(zip(X, Y, A))[::step]:
        ex, sc, _ = M.job_model(cm, x, y, a)
        n += int((sc["guards"] & window(ex, sc)).sum())
    return n


def _lists(rng, pool, reps=24, lens=(48, 64, 100), front=()):
    """reps accepted lists of each length drawn from `pool` in random order (the minimum lands in different lanes and late or early);
    `front`: variables every list starts with."""
    out = []
    for a in lens:
        for _ in range(reps):
            rest = [int(v) for v in rng.permutation([v for v in pool if v not in front])[:a - len(front)]]
            out.append(list(front) + rest)
    return out


# ---- matrices -----------------------------------------------------------------------------------------------------------------------
# Variables 0 and 1 are X and Y: they share a private component u, so X - Y stays strongly dependent given any three others.
def _near_collinear(m=112, seed=3):
    """Accepted variables are noisy copies of one factor g: v = g + s_v (e_v + l_v h), s_v in [0.045, 0.1] -- given ANY of them as z1 the
    others have sqrt(1 - cor^2) ~ sqrt(s_i^2 + s_v^2), so d1 = r_j r_k spans 0.004 ... 0.02 on both sides of the guard at 0.01.
    By construction INSENSITIVE to the size of dl: on this (positive-definite) matrix the model finds no size-3 test whose Float32
    estimate exceeds the exact |stat|^2 by more than the factor 1.0002 (critical scale 0), so a smaller dl skips nothing it must not.
    What the family checks is the kernel AT the guard d1 = 0.01 -- entries on either side in one wavefront step -- not dl."""
    rng = np.random.default_rng(seed)
    s, lam = rng.uniform(0.045, 0.1, m), rng.uniform(-0.6, 0.6, m)
    W, psi = np.zeros((2 + m, 3)), np.zeros(2 + m)  # latents g, u, h
    W[0], psi[0] = [0.5, 1.0, 0.4], 0.45
    W[1], psi[1] = [0.4, 1.0, 0.3], 0.5
    W[2:, 0], W[2:, 2], psi[2:] = 1.0, s * lam, s * s
    return M.cor_from_loadings(W, psi)


def _twins(m=112, seed=4):
    """Accepted variables in clusters of four around a cluster factor: within a cluster rho(v, w | z1) = 0.975 ... 0.995, i.e.
    g = 1 - F^2 between 0.01 and 0.05 on both sides of the guard at 0.02; across clusters F is small."""
    rng = np.random.default_rng(seed)
    nc = m // 4
    W, psi = np.zeros((2 + m, 2 + nc)), np.zeros(2 + m)  # latents u, common c, one per cluster
    W[0, :2], psi[0] = [1.0, 0.5], 0.4
    W[1, :2], psi[1] = [1.0, -0.4], 0.5
    W[0, 2:], W[1, 2:] = 0.25 * rng.standard_normal(nc), 0.25 * rng.standard_normal(nc)
    for v in range(m):
        W[2 + v, 1] = 0.3
        W[2 + v, 2 + v // 4] = 1.0
        psi[2 + v] = rng.uniform(0.005, 0.026)  # 1 - F^2 ~ 2 psi
    return M.cor_from_loadings(W, psi)


def _planar(m=112, seed=5):
    """X and every accepted variable lie, up to a little noise, in one three-dimensional space of factors: given z1 the rest is nearly
    planar, so the 3 x 3 determinant [X, zj, zk | z1] -- Pb -- is (X's height 0.015 over that space)^2 times the squared area zj and zk span:
    0 ... 2e-4 on both sides of dl = 1.2e-4, rho(X, zk | z1, zj) next to +-1 and, where round5 pushes it over, clamped.  X - Y does NOT stay
    dependent given any three here (a near-singular X leaves rho(X, Y | S) to the rounding noise): every job meets a non-significant
    test inside its first window.  What this family pins is the STOP -- status, num_tests, the stopping test's set and statistic -- in
    chunks whose other lanes are screened next to Pb = dl; a screen that skipped a non-significant test would move it."""
    rng = np.random.default_rng(seed)
    W, psi = np.zeros((2 + m, 4)), np.zeros(2 + m)  # latents h1, h2, h3, u
    d = rng.standard_normal((2 + m, 3))
    W[:, :3] = d / np.linalg.norm(d, axis=1)[:, None]
    psi[2:] = rng.uniform(0.001, 0.004, m) ** 2
    W[0, 3], psi[0] = 0.015, 0.002 ** 2
    W[1, :3] *= 0.6
    W[1, 3], psi[1] = 0.6, 0.25
    return M.cor_from_loadings(W, psi)


def _plateau(m=112, seed=6):
    """A hub g (variable 2) and accepted variables v = g + s (l_v h + e_v), l = 0.5, with sqrt(1 - cor(v, g)^2) = 0.104 (1 +- 1 %): with
    the hub as z1, d1 = 0.0103 ... 0.0112 and every test (hub, v, w) has the same |stat|^2 up to about 1e-3 relative -- C(a - 1, 2) >= 1 081
    of them, the job's smallest among them, wherever the random order of the list puts it.  The tests without the hub as z1 (d1 ~ 0.017)
    pass the guards as well and lie clearly above: the lanes the screen skips while the plateau's sit next to the bound.
    Like _near_collinear INSENSITIVE to the size of dl by construction (critical scale 0 for every test of it in the model): it pins the
    bookkeeping of a plateau -- bound published, neighbours within 1e-3 never skipped, minimum late and in any lane.  The plateau that a
    too-small dl breaks is the one of exact ties (_tie_blocks)."""
    rng = np.random.default_rng(seed)
    lam = 0.5 * (1.0 + 1e-2 * rng.standard_normal(m))
    r = 0.104 * (1.0 + 1e-2 * rng.standard_normal(m))
    s = r / np.sqrt(lam * lam + 1.0)
    W, psi = np.zeros((3 + m, 3)), np.zeros(3 + m)  # latents g, u, h
    W[0], psi[0] = [0.5, 1.0, 1.0], 0.45
    W[1], psi[1] = [-0.4, 1.0, 0.9], 0.5
    W[2] = [1.0, 0.0, 0.0]
    W[3:, 0], W[3:, 2], psi[3:] = 1.0, s * lam, s * s
    return M.cor_from_loadings(W, psi)


def _underflow(m=112, seed=7, n_med=10):
    """X = c + 0.05 e, Y = c + 0.05 e': rho(X, Y | S) ~ 0.997 and p underflows to 0 unless S holds mediators (noisy copies of c, the LAST
    n_med variables): one leaves p subnormal or 0, two or three bring |stat| to 0.95 ... 0.92 and p into the normal range."""
    rng = np.random.default_rng(seed)
    W, psi = np.zeros((2 + m, 2)), np.zeros(2 + m)  # latents c, b
    W[0, 0], W[1, 0], psi[0], psi[1] = 1.0, 1.0, 0.05 ** 2, 0.05 ** 2
    W[2:, 1], psi[2:] = 0.3 * rng.standard_normal(m), 1.0
    W[2 + m - n_med:, 0], psi[2 + m - n_med:] = 1.0, rng.uniform(0.25, 0.35, n_med) ** 2
    return M.cor_from_loadings(W, psi)


def _with_nan_columns(cm, k=3):
    """k more variables whose rows are NaN (zero-variance columns: Statistics.cor gives NaN off the unit diagonal)."""
    p = cm.shape[0]
    out = np.full((p + k, p + k), np.nan, dtype=f32)
    out[:p, :p] = cm
    out[np.arange(p + k), np.arange(p + k)] = 1.0
    return out


N_J, N_K = M.TIE_NJ, M.TIE_NK  # copies of zj / zk around one operand tuple: a list of 1 + 8 + 44 = 53; the last tied test (rank 379) lies in
# the second step of its wavefront, behind the bound the first step published (the job's first window, 256 ranks, is a segment of its own)


def _tie_blocks():
    """One block of 3 + 8 + 44 variables [X, Y, hub, J_1..8, K_1..44] (screen_model.tie_job_matrix) per operand tuple of
    tests/golden/screen_tuples.json (made by screen_model.select_tie_tuples): every test (hub, J_a, K_b) has the tuple's ten operands
    exactly, so N_J N_K = 352 tests per job TIE on the smallest |stat|^2 of the job -- on operands the directed search pushed onto round5
    half-points -- and the reference returns the LAST of them (tests.jl:338, `>=`)."""
    with open(os.path.join(GOLDEN, "screen_tuples.json")) as fh:
        tuples = json.load(fh)["tuples"]
    B = 3 + N_J + N_K
    cm = np.eye(B * len(tuples), dtype=f32)
    for b, t in enumerate(tuples):
        cm[b * B:(b + 1) * B, b * B:(b + 1) * B] = M.tie_job_matrix(t)
    return cm, len(tuples), B


def _q(ex):
    with np.errstate(all="ignore"):
        return ex["ev"] ** 2 / (ex["xb"] * ex["xc"])


# ---- the families ---------------------------------------------------------------------------------------------------------------------
_W = dict(
    near_collinear=lambda ex, sc: sc["d1"] < f32(0.02),                                   # d1 in (0.01, 0.02)
    twins=lambda ex, sc: sc["g"] < f32(0.05),                                             # g in (0.02, 0.05)
    planar=lambda ex, sc: (sc["Pb"] < 3.0 * sc["dl"]) | (sc["Pc"] < 3.0 * sc["dl"]),      # Pb or Pc in (dl, 3 dl)
    plateau=lambda ex, sc: sc["d1"] < f32(0.0115),                                        # the hub's tests
    underflow=lambda ex, sc: _q(ex) > M.fz_sure_range(N_OBS)[1],                          # p beyond the normal range: never a bound, may be skipped
    ties=lambda ex, sc: _q(ex) <= np.nanmin(_q(ex)) * (1.0 + 1e-12),                      # the tied minimum tests themselves
)


def _family(name):
    """-> (matrix, X, Y, accepted lists, every job runs to its last rank?)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "near_collinear":
        cm = _near_collinear()
        A = _lists(rng, range(2, cm.shape[0]))
    elif name == "twins":
        cm = _twins()
        A = _lists(rng, range(2, cm.shape[0]))
    elif name == "planar":  # (these jobs meet a non-significant test early: what counts is the first launch, 16 384 ranks a job)
        cm = _planar()
        A = _lists(rng, range(2, cm.shape[0]), reps=40, lens=(64, 100))
    elif name == "plateau":  # the hub first, third, or wherever the permutation puts it
        cm = _plateau()
        A = _lists(rng, range(3, cm.shape[0]), reps=12, front=(2,))
        for a in _lists(rng, range(3, cm.shape[0]), reps=12, front=(2,)):
            k = int(rng.integers(1, len(a) // 2))
            a[0], a[k] = a[k], a[0]
            A.append(a)
    elif name == "underflow":
        cm = _underflow()
        A = _lists(rng, range(2, cm.shape[0] - 10), lens=(40, 56, 92))
        # eight mediators behind the first ten variables: the job starts with p = 0; the rows (mediator, mediator, .) further on are whole
        # wavefront steps in the normal range of p (only those publish a bound), the single-mediator tests around them the lanes to skip
        A = [a[:10] + [int(v) for v in cm.shape[0] - 10 + rng.permutation(10)[:8]] + a[10:] for a in A]
    else:
        raise KeyError(name)
    return cm, [0] * len(A), [1] * len(A), A, name != "planar"


@pytest.mark.parametrize("name", ["near_collinear", "twins", "planar", "plateau", "underflow"])
def test_guard_window_family_equals_oracle(name):
    cm, X, Y, A, whole = _family(name)
    alens = [len(a) for a in A]
    nseg, rmin, rmax = _screen_segments(alens) if whole else _screen_segments(alens, max_tests=16384)
    cov = _coverage(cm, X, Y, A, _W[name])
    print("%s: %d jobs, %d ranks; size-3 segments with R >= 2: %d (R %d..%d); screened in window (sample of jobs): %d" %
          (name, len(A), sum(_job_ranks(a) for a in alens), nseg, rmin, rmax, cov))
    assert nseg >= 100 and cov >= 1000
    statuses, memo = _check_batch(cm, N_OBS, X, Y, A)
    if whole:  # (a condition on the inputs: every job all-significant, its maximum-p test among the size-3 tests)
        assert all(s == 2 for s in statuses)
        assert all(len(e["Zs"]) == 3 for e in memo.values())
    if name == "planar":  # (inputs: every job stops, inside its first window and inside size 3; most behind the first wavefront step)
        stops = sorted(e["num_tests"] for e in memo.values())
        print("planar: ranks before the stop: min %d, median %d, max %d" % (stops[0] - 1, stops[len(stops) // 2] - 1, stops[-1] - 1))
        assert all(s == 1 for s in statuses) and stops[-1] <= 16384
        assert sum(n > 64 for n in stops) >= 10
    if name == "plateau":
        assert all(2 in e["Zs"] for e in memo.values())  # ... and on the hub's plateau
    if name == "underflow":
        orc = O.Oracle("fz", cor_mat=cm, n_obs=N_OBS)
        assert all(orc.test(0, 1, a[:3])[1] == 0.0 for a in A[:5])  # the first test of a job: p = 0
        assert all(2.3e-308 < e["pval"] < 1e-100 for e in memo.values())


def test_round5_tie_plateaus_equal_oracle():
    """352 exactly tied minimum tests per job on the operand tuples of the directed search.  This is the family a too-small dl breaks
    (profiles/screen_directed.txt): with dl at one twentieth the screen skips later tied tests against the bound the first one published,
    and the job comes back with an earlier conditioning set."""
    cm, nt, B = _tie_blocks()
    rng = np.random.default_rng(99)
    X, Y, A = [], [], []
    for b in range(nt):
        o = b * B
        for _ in range(10):
            J, K = o + 3 + rng.permutation(N_J), o + 3 + N_J + rng.permutation(N_K)
            X.append(o), Y.append(o + 1), A.append([o + 2] + [int(v) for v in J] + [int(v) for v in K])
    nseg, rmin, rmax = _screen_segments([len(a) for a in A])
    cov = _coverage(cm, X, Y, A, _W["ties"], sample=24)
    print("ties: %d jobs; size-3 segments with R >= 2: %d (R %d..%d); tied minimum tests that pass every guard (sample of jobs): %d" % (len(A), nseg, rmin, rmax, cov))
    assert nseg >= 100 and cov >= 1000
    statuses, memo = _check_batch(cm, N_OBS, X, Y, A)
    assert all(s == 2 for s in statuses)
    for (x, y, a), e in memo.items():  # (inputs: the maximum-p test is the LAST of the tied tests (hub, J, K))
        assert e["Zs"] == (a[0], a[N_J], a[N_J + N_K]), (e, a[:8])


def test_nan_entries_next_to_clean_ones():
    """Accepted lists that hold one variable with a NaN row: the first test that touches it is not significant (NaN p) and ends the job, in a
    chunk whose other lanes are clean and screened.  Position 98 of 100: ranks 96, 97 + ..., the second step of the first wavefront."""
    cm = _with_nan_columns(_near_collinear(), 3)
    p = cm.shape[0]
    rng = np.random.default_rng(5)
    A = _lists(rng, range(2, p - 3), reps=30, lens=(100,))
    for i, a in enumerate(A):
        a[[98, 99, 70, 3][i % 4]] = p - 1 - i % 3
    A += _lists(rng, range(2, p - 3), reps=30, lens=(100,))  # clean jobs of the same launch
    nseg, _, _ = _screen_segments([len(a) for a in A], max_tests=16384)
    cov = _coverage(cm, [0] * 6, [1] * 6, A[30:36], _W["near_collinear"])
    assert nseg >= 100 and cov >= 1000
    statuses, _ = _check_batch(cm, N_OBS, [0] * len(A), [1] * len(A), A)
    assert statuses[:30] == [1] * 30 and statuses[30:] == [2] * 30


@pytest.mark.parametrize("on_minimum", [True, False])
def test_cap_inside_a_fast_loop_chunk(on_minimum):
    """max_tests ends the job inside a size-3 chunk of the fast loop (f_capped): the reference returns the test AT the cap (tests.jl:326-336),
    the one lane that must not be screened away.  on_minimum: the cap is the rank behind the smallest |stat|^2 of ranks [0, 12 600) -- the
    capped lane also holds the minimum the lanes next to it are screened against; else 77 ranks further.  100 copies of the job make the
    launch large enough for runs of two ranks per lane."""
    cm = _near_collinear()
    for seed in range(100):  # (a list whose smallest |stat|^2 of the first 12 600 ranks lies behind rank 8 000: 100 x cap > 786 432)
        a = _lists(np.random.default_rng(seed), range(2, cm.shape[0]), reps=1, lens=(100,))[0]
        ex, sc, pos = M.job_model(cm, 0, 1, a)
        with np.errstate(all="ignore"):
            q = ex["ev"] ** 2 / (ex["xb"] * ex["xc"])
        r_min = int(np.flatnonzero(q[:12600] == q[:12600].min())[-1])
        if r_min >= 8000:
            break
    assert 8000 <= r_min < 12600
    cap = r_min + 1 + (0 if on_minimum else 77)
    A = [list(a) for _ in range(100)] + _lists(np.random.default_rng(17), range(2, cm.shape[0]), reps=10, lens=(100,))
    nseg, _, _ = _screen_segments([len(x) for x in A], max_tests=cap)
    cov = int((sc["guards"][:cap] & _W["near_collinear"](ex, sc)[:cap]).sum())
    assert nseg >= 100 and cov >= 1000, (nseg, cov)
    statuses, memo = _check_batch(cm, N_OBS, [0] * len(A), [1] * len(A), A, max_tests=cap)
    e = memo[(0, 1, tuple(a))]
    assert e["status"] == 1 and e["num_tests"] == cap  # (inputs: the job ends on the cap, with the capped test's conditioning set)
    assert e["Zs"] == tuple(a[i] for i in pos[cap - 1])


# ---- the device-round path (fw_devhiton.hip): the same screen behind local matrices and transposed gathers ---------------------------
def _dense_factor_cor(p=128, core=50, k=8, seed=1):
    """50 of the 128 variables carry one factor, each with its own large noise (no three noisy copies pin it down: no pair among them is
    ever separated, their accepted lists grow to 48 and their PC sets to 49), and k weaker factors; the other 78 are independent noise
    (they only make two rounds of 64 targets, the fewest the device-round driver takes, affordable for the oracle)."""
    rng = np.random.default_rng(seed)
    W, psi = np.zeros((p, k + 1)), np.ones(p)
    idx = np.sort(rng.permutation(p)[:core])
    W[idx, 0], W[idx, 1:], psi[idx] = 1.0, 0.1 * rng.standard_normal((core, k)), rng.uniform(0.7, 1.1, core) ** 2
    return M.cor_from_loadings(W, psi)


def _cluster_cor(p=128, per=30, seed=2):
    """Three tight clusters of 30 noisy copies each (within a cluster cor ~ 0.97-0.995: d1 small) on one common factor, two exact duplicate
    columns (cor = 1: zero denominators, Float64 literals), and 38 variables of independent noise."""
    rng = np.random.default_rng(seed)
    W, psi = np.zeros((p, 4)), np.ones(p)
    idx = np.sort(rng.permutation(p)[:3 * per])
    for t, v in enumerate(idx):
        W[v, 0], W[v, 1 + t % 3], psi[v] = 0.8, 1.0, rng.uniform(0.08, 0.25) ** 2
    cm = M.cor_from_loadings(W, psi)
    a, b = idx[0], idx[3]  # (two members of the same cluster)
    cm[:, b], cm[b, :] = cm[:, a], cm[a, :]
    cm[b, b] = cm[a, b] = cm[b, a] = 1.0
    return cm


# No max_tests cap: a capped job returns the test AT the cap, and the screen's maximum-p decision could not reach an edge weight.  Here
# every job runs to its last rank or its first non-significant test, and what the screen decides is what the network holds.
ROUND_CASES = dict(dense=(_dense_factor_cor, 2000), clusters=(_cluster_cor, 2000))


@pytest.fixture(scope="module")
def round_cases():
    out = {}
    for name, (make, n) in ROUND_CASES.items():
        cm = make()
        out[name] = dict(cm=cm, n=n, orc=O.Oracle("fz", cor_mat=cm, n_obs=n))
    return out


@pytest.mark.parametrize("ff,R", [(True, 64), (False, 0)])
@pytest.mark.parametrize("name", ["dense", "clusters"])
def test_device_rounds_equal_oracle(round_cases, name, ff, R):
    """Engine.lgl against Oracle.learn as tests/test_gpu_fz_sched.py::_check_oracle: edge set, weights to the bit, reference-order test
    count -- with feed-forward (two rounds of 64 targets) and without (one round of 128), uncapped."""
    c = round_cases[name]
    p = c["cm"].shape[0]
    exp = c["orc"].learn(max_k=3, feed_forward=ff, round_size=max(R, 1) if ff else 1, threads=8)
    if name == "dense":
        # inputs: PC sets of 49, i.e. jobs over 48 accepted variables (the one-segment fast-loop length) that are significant to their
        # last rank -- status 2, the maximum-p test decides the edge weight.  Checked on the job that closes a target's list.
        off, idx = exp["pc_off"], exp["pc_idx"]
        long_ = [t for t in range(p) if off[t + 1] - off[t] >= 49]
        assert len(long_) >= 40
        for t in long_[:3]:
            pc = [int(v) for v in idx[off[t]:off[t + 1]]]
            e = c["orc"].test_subsets(t, pc[-1], pc[:-1], max_k=3, alpha=0.01, n_obs_min=20)
            assert len(pc) - 1 >= 48 and e["status"] == 2 and e["num_tests"] == _job_ranks(len(pc) - 1), e
    eng = fw.Engine("fz", c["n"], p, max_k=3)
    eng.set_cor_mat(c["cm"])
    net = eng.lgl(feed_forward=ff, round_size=R)
    cn = eng.counters()
    eng.close()
    print("%s ff=%s: %d edges, %d conditional tests, longest PC set %d; segment-kernel launches %d" %
          (name, ff, len(exp["edges"]), exp["n_cond_tests"], int(np.diff(exp["pc_off"]).max()), cn["subsets_launches"]))
    assert set(net["edges"]) == set(exp["edges"])
    for e, w in exp["edges"].items():
        assert net["edges"][e] == w
    assert cn["cond_tests_ref"] == exp["n_cond_tests"]
