"""The lean body of the size-3 Fisher-z table kernel (fw_fz_core.h: fz_seg3_lean_ok / fz_seg3_lean_body) on the device, through the C ABI
of the shipped library, against the oracle the way tests/test_gpu_fz_screen.py::_check_batch does (status, num_tests, Zs, stat exact;
pval, frac to 1e-12).

WHICH SEGMENTS TAKE IT.  _lean_ok restates fz_seg3_lean_ok on top of tests/pool_plan._plan (the host's segmenting): a segment [lo, hi)
of a job with a accepted variables is lean when 3 <= a <= 512, hi <= C(a, 3), no cap inside it (max_tests = 0 or hi < max_tests) and
p <= 46 000; everything else -- the segment that crosses C(a, 3), segments inside sizes 2 and 1, the segment that holds the cap, lists
without a size-3 subset -- keeps fz_seg_body.  Every case asserts, before anything is uploaded, that its batch holds the segments it is
about.  _plan is exact while no job ends before its last rank or the cap; where a case plants a stop it relies on the plan only up to
and including the launch that holds the stop (every job is still alive when that launch is cut).

WHAT A CASE PINS.  The lean body keeps chunks, table, mapping, screen, reductions and record of fz_seg_body; what is new is the control
flow around the step every lane passes.  So the cases put the events that LEAVE that step -- a non-significant test (a stop), a tie of
the maximum, an unclean (NaN) entry, a test inside the guard band of the significance threshold, a test beyond the normal range of p --
at chosen places of a lane's run (first step, last step, lane 0, lane 63, first and last wavefront), by rank, and check the job against
the oracle.  Lane l of wavefront w takes the ranks lo + 64 R w + l + 64 t, t < R, of a one-chunk segment (R = segment / 256).

The table-halving path (chunks of more than ~8 400 ranks at the end of a size-3 enumeration) cannot be reached through the host pool,
whose segments stop at 8 192 ranks; tests/test_gpu_fullsize.py -k cfg3 runs it.
"""
import itertools
import json
import math
import os

import numpy as np
import pytest

import flashweave_jl_amd as fw
from oracle import oracle as O
from tests import screen_model as M
from tests.pool_plan import _plan
from tests.test_gpu_fz_screen import N_J, N_K, N_OBS, _check_batch, _lists, _near_collinear, _tie_blocks, _underflow, _with_nan_columns
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

f32 = np.float32
TAB_A, P32_MAX = 512, 46000  # FW_TAB_A; p^2 < 2^31


# ---- the eligibility rule, restated ---------------------------------------------------------------------------------------------------
def _lean_ok(a, lo, hi, max_tests, p, max_k=3):
    if max_k < 3 or a < 3 or a > TAB_A:
        return False
    if hi > math.comb(a, 3):
        return False
    if max_tests > 0 and hi >= max_tests:
        return False
    return p <= P32_MAX


def _segments(alens, max_tests, p):
    """Every segment of the batch by the host's plan -> list of dict(job, launch, lo, hi, R, lean)."""
    out = []
    for li, (seglen, wins) in enumerate(_plan(alens, max_tests if max_tests > 0 else 1 << 62)):
        for i, lo, hi in wins:
            for s in range(lo, hi, seglen):
                e = min(hi, s + seglen)
                out.append(dict(job=i, launch=li, lo=s, hi=e, R=min(-(-(e - s) // 256), 64), lean=_lean_ok(alens[i], s, e, max_tests, p)))
    return out


def _segment_of(segs, job, rank):
    (sg,) = [s for s in segs if s["job"] == job and s["lo"] <= rank < s["hi"]]
    return sg


def _where(sg, rank):
    """(wavefront, lane, step) of a rank inside a one-chunk segment."""
    rel = rank - sg["lo"]
    w, r = divmod(rel, 64 * sg["R"])
    return w, r % 64, r // 64


# ---- matrices -------------------------------------------------------------------------------------------------------------------------
S1, S2, S3 = 2, 3, 4  # the planted triple


def _planted_cor(m=120, seed=11, s_noise=1e-4):
    """X = s1 + s2 + s3 + noise, Y likewise; variables 2, 3, 4 are s1, s2, s3 (up to s_noise) and the m others junk on a factor of their
    own with a little of s1..s3 each: rho(X, Y | S) is 0.5 ... 0.9 -- significant for sure, normal range of p, clean -- for every S of up
    to three variables EXCEPT S = {s1, s2, s3}, which leaves nothing: ONE non-significant size-3 test per list that holds all three, at the
    rank its positions give it."""
    rng = np.random.default_rng(seed)
    W, psi = np.zeros((5 + m, 4)), np.ones(5 + m)
    W[0, :3], psi[0] = 1.0, 0.5
    W[1, :3], psi[1] = 1.0, 0.6
    for i in range(3):
        W[2 + i, i], psi[2 + i] = 1.0, s_noise
    W[5:, 3], W[5:, :3] = 0.5, 0.15 * rng.standard_normal((m, 3))
    return M.cor_from_loadings(W, psi)


def _triple_at(a, rank):
    """Positions (i, j, k) of rank `rank` of the size-3 enumeration of a list of a variables (lexicographic)."""
    return next(itertools.islice(itertools.combinations(range(a), 3), rank, None))


def _plant(base, rank):
    """The list `base` (junk only) with s1, s2, s3 at the positions of rank `rank`."""
    a = list(base)
    for q, v in zip(_triple_at(len(a), rank), (S1, S2, S3)):
        a[q] = v
    return a


# ---- 1. both bodies in one launch ---------------------------------------------------------------------------------------------------------
def test_both_bodies_in_one_launch():
    cm = _near_collinear()
    p = cm.shape[0]
    rng = np.random.default_rng(21)
    A = _lists(rng, range(2, p), reps=24) + _lists(rng, range(2, p), reps=2, lens=(2, 3, 9))
    alens = [len(a) for a in A]
    cap = 150_000  # inside the size-3 enumeration of the lists of 100 (C(100, 3) = 161 700), beyond the last rank of every other list
    segs = _segments(alens, cap, p)
    c3 = lambda s: math.comb(alens[s["job"]], 3)
    kinds = dict(lean=[s for s in segs if s["lean"]],
                 crosses=[s for s in segs if 3 <= alens[s["job"]] and s["lo"] < c3(s) < s["hi"]],
                 sizes21=[s for s in segs if alens[s["job"]] >= 3 and s["lo"] >= c3(s)],
                 cap=[s for s in segs if s["hi"] == cap],
                 short=[s for s in segs if alens[s["job"]] < 3])
    print({k: len(v) for k, v in kinds.items()}, "R of the lean segments:", sorted({s["R"] for s in kinds["lean"]}))
    assert len(kinds["lean"]) >= 100 and max(s["R"] for s in kinds["lean"]) >= 2
    for k in ("crosses", "sizes21", "cap", "short"):
        assert kinds[k] and not any(s["lean"] for s in kinds[k]), k
    last = max(s["launch"] for s in segs)  # ONE launch holds lean segments next to a crossing one, one inside sizes 2 and 1 and a capped one
    for k in ("lean", "crosses", "sizes21", "cap"):
        assert any(s["launch"] == last for s in kinds[k]), k
    statuses, memo = _check_batch(cm, N_OBS, [0] * len(A), [1] * len(A), A, max_tests=cap)
    for a, st in zip(A, statuses):  # (inputs: every job runs to its last rank or to the cap -- the plan above is the host's)
        e = memo[(0, 1, tuple(a))]
        assert (st, e["num_tests"]) == ((1, cap) if len(a) == 100 else (2, math.comb(len(a), 3) + math.comb(len(a), 2) + len(a))), (len(a), e)


# ---- 2. eligibility edges -----------------------------------------------------------------------------------------------------------------
C20 = math.comb(20, 3)  # 1 140: alone in a launch a job is cut into segments of 256 ranks -- [0, 256) ... [768, 1024), [1024, ...)


@pytest.mark.parametrize("a,max_tests,lean_los,other_los", [
    (20, C20, [0, 256, 512, 768], [1024]),       # the last size-3 segment ends ON the cap: not lean
    (20, C20 + 1, [0, 256, 512, 768], [1024]),   # ... holds the cap and crosses C(a, 3)
    (20, 900, [0, 256, 512], [768]),             # the cap in the middle of a segment that lies wholly inside size 3
    (20, 0, [0, 256, 512, 768], [1024, 1280]),   # no cap: [1024, 1280) crosses C(a, 3), [1280, 1350) is sizes 2 and 1
    (3, 0, [], [0]),                             # the single size-3 subset sits in a segment that runs on into size 2
    (12, 0, [], [0, 256]),                       # C(12, 3) = 220 < 256: the first segment already crosses
    (13, 0, [0], [256]),                         # C(13, 3) = 286: the smallest list with a lean segment under the host's plan
])
def test_eligibility_edges(a, max_tests, lean_los, other_los):
    cm = _near_collinear()
    p = cm.shape[0]
    A = _lists(np.random.default_rng(31 + a), range(2, p), reps=6, lens=(a,))
    segs = _segments([a] * len(A), max_tests, p)
    for j in range(len(A)):
        assert sorted(s["lo"] for s in segs if s["job"] == j and s["lean"]) == lean_los
        assert sorted(s["lo"] for s in segs if s["job"] == j and not s["lean"]) == other_los
    statuses, memo = _check_batch(cm, N_OBS, [0] * len(A), [1] * len(A), A, max_tests=max_tests)
    n_all = math.comb(a, 3) + math.comb(a, 2) + a
    for e in memo.values():  # (inputs: all-significant lists -- every job runs to the cap or to its last rank)
        assert (e["status"], e["num_tests"]) == ((1, max_tests) if 0 < max_tests <= n_all else (2, n_all)), e


# ---- 3. every way out of the inner loop, and back in ------------------------------------------------------------------------------------------
def _planted_batch():
    cm = _planted_cor()
    p = cm.shape[0]
    rng = np.random.default_rng(41)
    A = _lists(rng, range(5, p), reps=24)
    bases = _lists(rng, range(5, p), reps=8, lens=(100,))
    return cm, p, A, bases


def test_planted_stop_at_chosen_places_of_a_run():
    """One non-significant size-3 test per planted job, at the first and the last step of a lane's run, in lane 0 and lane 63, in the first
    wavefront (later ranks of the segment already evaluated by the other three) and in the last."""
    cm, p, A, bases = _planted_batch()
    n0 = len(A)
    alens = [len(a) for a in A] + [100] * len(bases)
    segs = _segments(alens, 10_000_000, p)
    last = max(s["launch"] for s in segs)
    places, want = [], []
    for j, base in enumerate(bases):
        sg = [s for s in segs if s["job"] == n0 + j and s["launch"] == last][3 + j]  # a segment of the last launch, a different one per job
        R = sg["R"]
        assert sg["lean"] and R >= 2 and sg["hi"] - sg["lo"] == 256 * R
        w, l, t = [(0, 5, 0), (1, 9, R - 1), (2, 0, 1), (1, 63, 1), (3, 17, R // 2), (0, 30, 1), (3, 63, R - 1), (0, 0, 0)][j]
        rank = sg["lo"] + 64 * R * w + l + 64 * t
        assert _where(sg, rank) == (w, l, t)
        places.append((w, l, t, R))
        want.append(rank)
        A.append(_plant(base, rank))
    print("planted (wavefront, lane, step, R):", places)
    statuses, memo = _check_batch(cm, N_OBS, [0] * len(A), [1] * len(A), A)
    assert all(s == 2 for s in statuses[:n0])  # (inputs: the unplanted jobs are all-significant -- the plan is the host's)
    for a, rank in zip(A[n0:], want):  # from the oracle's values: the planted test exists, at its rank
        e = memo[(0, 1, tuple(a))]
        assert e["status"] == 1 and e["num_tests"] == rank + 1 and e["Zs"] == (S1, S2, S3), (rank, e)


def test_tie_of_the_maximum_between_two_wavefronts():
    """The 352 exactly tied minimum tests of a tie job (tests/test_gpu_fz_screen.py::_tie_blocks) with few jobs in the launch: segments of
    256 ranks, one test per lane -- the tied tests of ranks 256 ... 379 lie in the first TWO wavefronts of the lean segment [256, 512), and
    the later rank wins (tests.jl:338)."""
    cm, nt, B = _tie_blocks()
    rng = np.random.default_rng(51)
    X, Y, A = [], [], []
    for b in range(nt):
        o = b * B
        J, K = o + 3 + rng.permutation(N_J), o + 3 + N_J + rng.permutation(N_K)
        X.append(o), Y.append(o + 1), A.append([o + 2] + [int(v) for v in J] + [int(v) for v in K])
    segs = _segments([len(a) for a in A], 10_000_000, cm.shape[0])
    for j, (x, y, a) in enumerate(zip(X, Y, A)):
        ex, _, _ = M.job_model(cm, x, y, a)
        with np.errstate(all="ignore"):
            q = ex["ev"] ** 2 / (ex["xb"] * ex["xc"])
        tied = np.flatnonzero(q == np.nanmin(q))
        sg = _segment_of(segs, j, int(tied[-1]))
        assert sg["lean"] and (sg["lo"], sg["hi"], sg["R"]) == (256, 512, 1)
        waves = {_where(sg, int(r))[0] for r in tied if sg["lo"] <= r < sg["hi"]}
        assert waves == {0, 1} and _where(sg, int(tied[-1]))[0] == 1, (waves, tied[-1])
    statuses, memo = _check_batch(cm, N_OBS, X, Y, A)
    assert all(s == 2 for s in statuses)
    for (x, y, a), e in memo.items():
        assert e["Zs"] == (a[0], a[N_J], a[N_J + N_K]), (e, a[:8])


def test_nan_column_inside_clean_lists():
    """One variable with a NaN row at position 98 of 100: rank 96 -- (0, 1, 98) -- is the first test that touches it, not significant
    (NaN p), in a lean segment whose other entries are clean."""
    cm = _with_nan_columns(_near_collinear(), 3)
    p = cm.shape[0]
    rng = np.random.default_rng(61)
    A = _lists(rng, range(2, p - 3), reps=60, lens=(100,))
    for i in range(12):
        A[i][98] = p - 1 - i % 3
    segs = _segments([100] * len(A), 10_000_000, p)
    sg = _segment_of([s for s in segs if s["launch"] == 0], 0, 96)
    assert sg["lean"] and sg["R"] >= 2 and _triple_at(100, 96) == (0, 1, 98)
    print("NaN: rank 96 is (wavefront, lane, step) = %s of a segment with R = %d" % (_where(sg, 96), sg["R"]))
    statuses, memo = _check_batch(cm, N_OBS, [0] * len(A), [1] * len(A), A)
    assert statuses == [1] * 12 + [2] * (len(A) - 12)
    for a in A[:12]:
        e = memo[(0, 1, tuple(a))]
        assert e["num_tests"] == 97 and np.isnan(e["pval"]) and e["Zs"] == (a[0], a[1], a[98])


def _guard_band_threshold(n_obs=N_OBS):
    # |stat| at which p = alpha = 0.01 (the p-value's scale is sqrt(n_obs - 3) / 2 whatever the size of the set); the band is +-1e-9 around it
    return math.sqrt(M.fz_sure_range(n_obs, n_cond=0)[0])


def _guard_band_cor():
    """_planted_cor with s1..s3 noisy enough that rho(X, Y | s1, s2, s3) sits next to the significance threshold, and the ten matrix
    entries of that test replaced by the Float32 values of tests/golden/lean3_guard_band.json: found by walking those ten entries a few
    ulps at a time under tests/screen_model.exact until |stat| lay within 1e-10 (relative) of the threshold -- inside the kernel's
    +-1e-9 guard band, where the exact p-value decides (fz_pval_slow) instead of the thresholds on |r|."""
    with open(os.path.join(GOLDEN, "lean3_guard_band.json")) as fh:
        g = json.load(fh)
    cm = _planted_cor(s_noise=g["s_noise"])
    for u, v, x in g["entries"]:
        cm[u, v] = cm[v, u] = f32(float.fromhex(x))
    return cm


def test_guard_band_of_the_significance_threshold():
    cm = _guard_band_cor()
    p = cm.shape[0]
    rng = np.random.default_rng(71)
    A = _lists(rng, range(5, p), reps=24)
    bases = _lists(rng, range(5, p), reps=2, lens=(100,))
    n0 = len(A)
    alens = [len(a) for a in A] + [100] * len(bases)
    segs = _segments(alens, 10_000_000, p)
    last = max(s["launch"] for s in segs)
    want = []
    for j, base in enumerate(bases):
        sg = [s for s in segs if s["job"] == n0 + j and s["launch"] == last][5 + j]
        assert sg["lean"] and sg["R"] >= 2
        rank = sg["lo"] + 64 * sg["R"] * (1 + j) + 40 + 64 * j
        want.append(rank)
        A.append(_plant(base, rank))
    orc = O.Oracle("fz", cor_mat=cm, n_obs=N_OBS)
    stat, pval = orc.test(0, 1, [S1, S2, S3])[:2]
    orc.close()
    thr = _guard_band_threshold()
    print("guard band: |stat| / threshold - 1 = %.3g, p = %.17g" % (abs(stat) / thr - 1.0, pval))
    # from the oracle's values: the planted test lies inside the guard band, its p next to alpha
    assert abs(abs(stat) / thr - 1.0) < 5e-10 and abs(pval / 0.01 - 1.0) < 1e-7
    statuses, memo = _check_batch(cm, N_OBS, [0] * len(A), [1] * len(A), A)
    assert all(s == 2 for s in statuses[:n0])
    for a, rank in zip(A[n0:], want):  # significant or not is the exact p-value's call: the oracle's, either way at this rank
        e = memo[(0, 1, tuple(a))]
        if pval < 0.01:
            assert e["status"] == 2
        else:
            assert e["status"] == 1 and e["num_tests"] == rank + 1 and e["Zs"] == (S1, S2, S3), (rank, e)


def test_beyond_the_normal_range_of_p():
    """Jobs that start with p = 0 (tests/test_gpu_fz_screen.py::_underflow): the first ranks of a lean segment lie beyond the normal range
    of p, where the maximum-p bookkeeping orders by the exact p."""
    cm = _underflow()
    p = cm.shape[0]
    rng = np.random.default_rng(81)
    A = _lists(rng, range(2, p - 10), lens=(40, 56, 92))
    A = [a[:10] + [int(v) for v in p - 10 + rng.permutation(10)[:8]] + a[10:] for a in A]
    segs = _segments([len(a) for a in A], 10_000_000, p)
    assert all(_segment_of(segs, j, 0)["lean"] for j in range(len(A)))
    assert sum(s["lean"] and s["R"] >= 2 for s in segs) >= 100
    orc = O.Oracle("fz", cor_mat=cm, n_obs=N_OBS)
    assert all(orc.test(0, 1, a[:3])[1] == 0.0 for a in A[::8])  # from the oracle's values: rank 0 of a job has p = 0
    orc.close()
    statuses, memo = _check_batch(cm, N_OBS, [0] * len(A), [1] * len(A), A)
    assert all(s == 2 for s in statuses)
    assert all(2.3e-308 < e["pval"] < 1e-100 for e in memo.values())


# ---- 4. device rounds: the local-matrix form (FwSeg::tm != 0) ------------------------------------------------------------------------------
def _star_cor(p=128, leaves=70, seed=5):
    """One hub and 70 noisy copies of it (each with its own noise level: no exact ties) among independent noise: the hub keeps all 70
    neighbours -- its jobs run over up to 69 accepted variables, every size-3 test significant -- while a leaf loses every other leaf
    to the hub at size 1, so the network costs the oracle a second."""
    rng = np.random.default_rng(seed)
    W, psi = np.zeros((p, 1)), np.ones(p)
    idx = np.sort(rng.permutation(p)[:leaves + 1])
    hub = int(idx[leaves // 2])
    W[idx, 0], psi[idx] = 1.0, rng.uniform(0.7, 1.1, leaves + 1) ** 2
    psi[hub] = 1e-6
    return M.cor_from_loadings(W, psi), hub


@pytest.fixture(scope="module")
def hub_case():
    cm, hub = _star_cor()
    return dict(cm=cm, hub=hub, n=2000, orc=O.Oracle("fz", cor_mat=cm, n_obs=2000))


@pytest.mark.parametrize("ff,R", [(True, 64), (False, 0)])
def test_device_rounds_with_a_hub_equal_oracle(hub_case, ff, R):
    """Engine.lgl against Oracle.learn as tests/test_gpu_fz_screen.py::test_device_rounds_equal_oracle, on a network whose hubs keep 64 and
    more neighbours: its jobs are cut into segments of the local-matrix form, lean inside size 3."""
    c = hub_case
    p = c["cm"].shape[0]
    exp = c["orc"].learn(max_k=3, feed_forward=ff, round_size=max(R, 1) if ff else 1, threads=8)
    deg = np.diff(exp["pc_off"])
    longest = int(deg.max())
    assert longest >= 65 and int(np.argmax(deg)) == c["hub"]  # from the oracle's network: the hub keeps >= 64 neighbours besides a candidate
    eng = fw.Engine("fz", c["n"], p, max_k=3)
    eng.set_cor_mat(c["cm"])
    net = eng.lgl(feed_forward=ff, round_size=R)
    cn = eng.counters()
    eng.close()
    print("hub ff=%s: %d edges, %d conditional tests, longest PC set %d" % (ff, len(exp["edges"]), exp["n_cond_tests"], longest))
    assert set(net["edges"]) == set(exp["edges"])
    for e, w in exp["edges"].items():
        assert net["edges"][e] == w
    assert cn["cond_tests_ref"] == exp["n_cond_tests"]
