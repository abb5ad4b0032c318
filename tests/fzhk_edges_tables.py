"""Tables, a model of the kernel's chunk walks and the job lists shared by tests/test_fzhk_edges_cpu.py, tests/test_gpu_fzhk_edges.py and
tests/fzhk_edges_worker.py: the max_k 4-5 Fisher-z segment kernels (csrc/fw_fz_core.h: fz_seg_body<HIGHK, ., .>) at every list-length,
table and chunk switch.  numpy only, no GPU import; every generator is seeded by its arguments, so the CPU module, the GPU module and a
child process hold the same bytes.

A job is (T = 0, candidate = 1, accepted list) on the correlation matrix of one generated table.  The generators plant WHERE a job ends:
`planted` tables stop it at one chosen rank of the enumeration, `leaky` tables put the maximum p there.  The model (pool plan + chunk
walks) only chooses ranks and says which switch a job sits on; what is right is decided by the oracle alone."""
import collections
import functools
import math

import numpy as np

from tests.pool_plan import _job_ranks, _plan

# ---- the constants of the switch points (tests/test_fzhk_edges_cpu.py holds them to the #defines: file, name, value) ----
DEFINES = """
fw_internal.h   FW_HK_A         88
fw_fz_core.h    FZ_L1_A         512
fw_fz_core.h    FW_ACC_LDS      2048
fw_unrank.h     FW_UNRANK32_A5  128
fw_fz_core.h    FZ_HK_CAP       4096
fw_fz_core.h    FZ_HK_DIR       96
fw_fz_core.h    FZ_L3_CAP       448
fw_fz_core.h    FZ_L3_DIR       64
fw_fz_core.h    FW_RUN_MAX      32
fw_fz_core.h    FZ_X_SUB        26.0
fw_fz_core.h    FW_L3_ENTRY_NN  1
"""
(HK_A, L1_A, ACC_LDS, UNRANK32_A5, HK_CAP, HK_DIR, L3_CAP, L3_DIR, RUN_MAX, X_SUB, L3_ENTRY_NN) = (
    float(ln.split()[2]) if "." in ln.split()[2] else int(ln.split()[2]) for ln in DEFINES.strip().splitlines())  # in the order of the rows
CHUNK = 256 * RUN_MAX           # the longest chunk, and the longest segment of the host pool
W0_SMALL, W0_BIG, W0_A = 256, 16384, 64  # first window (fw_pool_first_window)
N_ROWS = 4000
ALPHA = 0.01
MAX_TESTS = 10_000_000
C = math.comb


# ---- the enumeration: sizes max_k .. 1, lexicographic inside a size (tests.jl:281-346) ----
def size_of(rank, a, max_k):
    """-> (subset size at this rank, rank inside that size's enumeration)"""
    s = max_k
    while s > 1 and rank >= C(a, s):
        rank -= C(a, s)
        s -= 1
    return s, rank


def unrank_comb(rem, a, s):
    pos, prev = [], -1
    for d in range(s):
        t = s - d
        c = prev + 1
        while rem >= C(a - 1 - c, t - 1):
            rem -= C(a - 1 - c, t - 1)
            c += 1
        pos.append(c)
        prev = c
    return pos


def unrank(rank, a, max_k):
    s, rem = size_of(rank, a, max_k)
    return unrank_comb(rem, a, s)


def rank_of(pos, a, max_k):
    s = len(pos)
    r = sum(C(a, t) for t in range(s + 1, max_k + 1))
    prev = -1
    for d, q in enumerate(pos):
        r += sum(C(a - 1 - c, s - d - 1) for c in range(prev + 1, q))
        prev = q
    return r


def first_rank(a, max_k, s):
    """rank of the first subset of s variables"""
    return sum(C(a, t) for t in range(s + 1, max_k + 1))


# ---- tables ----
def _cor32(data):
    """Pearson matrix of a Float32 table: Float64 sums, rounded to Float32, mirrored, unit diagonal; a constant column gives a NaN row."""
    d = data.astype(np.float64)
    d = d - d.mean(axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = d / np.sqrt((d * d).sum(axis=0))
        cm = np.clip(d.T @ d, -1.0, 1.0).astype(np.float32)
    cm = np.minimum(cm, cm.T)  # exactly symmetric (NaN on both sides)
    np.fill_diagonal(cm, 1.0)
    cm = np.asfortranarray(cm)
    cm.setflags(write=False)
    return cm


COLLIDE = 0.25
SALT = {(37, 4, 0.0, 0.0, "twin"): 1}  # seed 9001: the planted partial correlation rounds to 0.0 in five digits (p = 1: nothing to compare)
N_ROWS_COLLIDE = 40000


def rows_of(key):
    """sample count of table(*key): the colliding tables need a finer test (see table)"""
    return N_ROWS_COLLIDE if key[3] > 0 else N_ROWS


@functools.lru_cache(maxsize=None)
def table(b, k, leak=0.0, collide=0.0, variant=""):
    """-> Float32 correlation matrix over [X, Y, S_0 .. S_{k-1}, b bystanders].  X = sum(S) + 0.7 noise + leak g, Y likewise with the
    same hidden g: X and Y are independent given all of S (leak = 0), and dependent given anything less.  The bystanders share a weak
    factor.  collide > 0: every bystander is also a weak child of X + Y, so conditioning on S AND a bystander makes X and Y dependent
    again (rho about -0.027 per bystander: 40 000 rows, threshold 0.013) -- S stops the job although |S| < max_k; five such
    bystanders alone are far too weak a proxy of X + Y to cancel the correlation S leaves.  variant "twin": the last bystander is a
    copy of the one before it (cor = 1.0 exactly); "const": the last bystander is constant (a NaN row)."""
    salt = SALT.get((b, k, leak, collide, variant), 0)
    rng = np.random.default_rng([9001 + salt, b, k, int(round(1000 * leak)), int(round(1000 * collide)), len(variant)])
    n = N_ROWS_COLLIDE if collide > 0 else N_ROWS
    S = rng.standard_normal((n, k))
    g = rng.standard_normal(n)
    x = S.sum(axis=1) + 0.7 * rng.standard_normal(n) + leak * g
    y = S.sum(axis=1) + 0.7 * rng.standard_normal(n) + leak * g
    B = 0.3 * rng.standard_normal((n, 1)) + rng.standard_normal((n, b)) + collide * (x + y)[:, None]
    data = np.concatenate([x[:, None], y[:, None], S, B], axis=1).astype(np.float32)
    if variant == "twin":
        data[:, -1] = data[:, -2]
    elif variant == "const":
        data[:, -1] = np.float32(1.5)
    else:
        assert variant == ""
    return _cor32(data)


def make_list(a, placed, fillers):
    """accepted list of a variables: placed = {position: id}, the other positions take `fillers` in order"""
    out, it = [], iter(fillers)
    for q in range(a):
        out.append(placed[q] if q in placed else next(it))
    assert len(set(out)) == a
    return tuple(out)


Job = collections.namedtuple("Job", "a rank acc expect why")   # expect: "stop" | "max" | "nan" | "last"; rank: where it ends / its maximum
Batch = collections.namedtuple("Batch", "name key max_k n_obs jobs")  # key: arguments of table(); one Engine / one Oracle per batch


def planted_job(key, max_k, a, rank, why=""):
    """S at the positions unranked from `rank` (|S| = the table's k = the subset size there), bystanders elsewhere"""
    b, k = key[0], key[1]
    pos = unrank(rank, a, max_k)
    assert len(pos) == k and a - k <= b, (key, max_k, a, rank, pos)
    placed = {q: 2 + t for t, q in enumerate(pos)}
    return Job(a, rank, make_list(a, placed, range(2 + k, 2 + k + b)), "max" if key[2] > 0 else "stop", why)


def zs_of(job, max_k):
    """the conditioning set the job must return"""
    return tuple(job.acc[q] for q in unrank(job.rank, job.a, max_k))


# ---- the model: host plan and the two directory walks ----
def plan_of(batch, seg_target=0):
    """-> per job the list of its segments [(start, end)] in rank order, up to and including the window its end lies in"""
    alens = [j.a for j in batch.jobs]
    stops = [j.rank if j.expect in ("stop", "nan") else None for j in batch.jobs]
    segs = [[] for _ in alens]
    for seglen, wins in _plan(alens, MAX_TESTS, batch.max_k, stops, seg_target):
        for i, lo, hi in wins:
            segs[i] += [(s, min(hi, s + seglen)) for s in range(lo, hi, seglen)]
    return segs


def _hk_entries(n):
    return 1 + 2 * n + n * (n - 1) // 2


def _hk_walk(a, s0, rem0, seg_left):
    """level-2 directory walk of one chunk (fz_seg_body, `if (HK)`) -> (chunk length, reason)"""
    i, j = unrank_comb(rem0, a, s0)[:2]
    tests = lambda n: C(n, s0 - 2)
    cur_end = (C(a, s0) - C(a - i, s0)) + (C(a - 1 - i, s0 - 1) - C(a - j, s0 - 1)) + tests(a - 1 - j)
    lim, reason = min(((rem0 + seg_left, "segment"), (C(a, s0), "size"), (rem0 + CHUNK, "run")), key=lambda v: v[0])
    nd = eoff = 0
    while True:
        e = _hk_entries(a - 1 - j)
        if nd > 0 and eoff + e > HK_CAP:
            lim, reason = cur_end - tests(a - 1 - j), "cap"
            break
        eoff += e
        nd += 1
        if cur_end >= lim:
            break
        if nd == HK_DIR:
            lim, reason = cur_end, "dir"
            break
        j += 1
        if j > a - s0 + 1:
            i += 1
            j = i + 1
        cur_end += tests(a - 1 - j)
    return lim - rem0, reason


def _l3_walk(a, s0, rem0, clen):
    """level-3 directory walk of one chunk inside one z1-block -> (chunk length, reason | None, "big" | "")"""
    i, j, k, l0 = unrank_comb(rem0, a, s0)[:4]
    t3 = s0 - 3
    cur_end = (C(a, s0) - C(a - i, s0)) + (C(a - 1 - i, s0 - 1) - C(a - j, s0 - 1)) + (C(a - 1 - j, s0 - 2) - C(a - k, s0 - 2)) + C(a - 1 - k, t3)
    lim, reason = rem0 + clen, None
    nd = eoff = 0
    while True:
        lo_w = l0 if nd == 0 else k + 1
        ne = a - lo_w
        if eoff + ne > L3_CAP:
            if nd == 0:
                return clen, None, "big"
            lim, reason = cur_end - C(a - 1 - k, t3), "cap"
            break
        eoff += ne
        nd += 1
        if cur_end >= lim:
            break
        if nd == L3_DIR:
            lim, reason = cur_end, "dir"
            break
        k += 1
        if k > a - s0 + 2:
            j += 1
            k = j + 1
        cur_end += C(a - 1 - k, t3)
    return lim - rem0, reason, ""


Chunk = collections.namedtuple("Chunk", "lo hi form reason")
# form: l2 (level-2 tables) | l3 (level-3 position tables) | l1 (level-1 table only: one sub-block too large) | plain_size (long list: the
# chunk spans a size change) | plain_z1 (... two z1-blocks) | gather (lists beyond 512) | inlane (sizes <= 3)
# reason the chunk ends: segment | run | size | cap | dir


def chunks(a, max_k, start, end):
    """The chunks fz_seg_body cuts the segment [start, end) into, for a list of a variables on the host pool's routing."""
    R = min(-(-(end - start) // 256), RUN_MAX)
    out, cbase = [], start
    while cbase < end:
        cend = min(cbase + 256 * R, end)
        reason = "segment" if cend == end else "run"
        s0, rem0 = size_of(cbase, a, max_k)
        form = "inlane" if s0 <= 3 else "gather"
        if s0 >= 4 and a <= HK_A:
            clen, reason = _hk_walk(a, s0, rem0, end - cbase)
            cend, form = cbase + clen, "l2"
        elif s0 >= 4 and a <= L1_A:
            if rem0 + (cend - cbase) > C(a, s0):
                form = "plain_size"
            elif unrank_comb(rem0, a, s0)[0] != unrank_comb(rem0 + (cend - cbase) - 1, a, s0)[0]:
                form = "plain_z1"
            else:
                clen, r3, big = _l3_walk(a, s0, rem0, cend - cbase)
                form = "l1" if big else "l3"
                if r3:
                    cend, reason = cbase + clen, r3
        out.append(Chunk(cbase, cend, form, reason))
        cbase = cend
    return out


def where(batch, seg_target=0):
    """-> per job (segment, chunks of that segment, index of the chunk that holds job.rank)"""
    out = []
    for job, segs in zip(batch.jobs, plan_of(batch, seg_target)):
        seg = next(s for s in segs if s[0] <= job.rank < s[1])
        ch = chunks(job.a, batch.max_k, *seg)
        out.append((seg, ch, next(i for i, c in enumerate(ch) if c.lo <= job.rank < c.hi)))
    return out


def coverage(batches, seg_target=0):
    """-> set of (form, reason, side): a job ends on the last rank of a chunk of that form that ends for that reason ("last"), or on the
    first rank behind one ("first": form and reason of the chunk in front; a segment's first rank: the form of its own chunk, reason
    "segment"); and (form, "inside", "") for every form a job's rank lies in."""
    got = set()
    for b in batches:
        for job, (seg, ch, i) in zip(b.jobs, where(b, seg_target)):
            c = ch[i]
            got.add((c.form, "inside", ""))
            if job.rank == c.hi - 1:
                got.add((c.form, c.reason, "last"))
            if job.rank == c.lo:
                got.add((ch[i - 1].form, ch[i - 1].reason, "first") if i else (c.form, "segment", "first"))
    return got


def model_ends(a, max_k, lo, hi, form, reason, seglen=CHUNK):
    """Chunk ends of that form and reason in [lo, hi), with the job cut into segments of `seglen` ranks the way the host pool cuts its
    windows (every window edge is a multiple of 8 192 ranks behind the first window: 256 ranks for lists under 64 variables)."""
    origin = 0 if a >= W0_A else W0_SMALL
    N = _job_ranks(a, MAX_TESTS, max_k)
    out = []
    s = origin + (max(lo, origin) - origin) // seglen * seglen
    while s < min(hi, N):
        out += [c.hi for c in chunks(a, max_k, s, min(N, s + seglen)) if c.form == form and c.reason == reason and lo <= c.hi < hi]
        s += seglen
    return out


# ---- job lists ----
def _around(e):
    return (e - 1, e, e + 1)


def _dedup(ranks, N):
    return sorted({r for r in ranks if 0 <= r < N})


LEN_SWITCH_A = (88, 89, 128, 129, 130, 131, 512, 513, 2048, 2049)
SHALLOW = (0, 255, 256, 8191, 8192, 16383, 16384, 16385)
BIG_B = 2049 - 4          # bystanders of the table the list-length family shares: room for a = 2049 at k = 4
MID_B = 452 - 4


@functools.lru_cache(maxsize=None)
def family_lengths(max_k):
    """1. every routing switch by list length x planted stops on both sides of the first chunk, segment and window ends"""
    key = (BIG_B, max_k, 0.0, 0.0, "")
    jobs = [planted_job(key, max_k, a, r, "a=%d" % a) for a in LEN_SWITCH_A for r in SHALLOW]
    return [Batch("lengths", key, max_k, N_ROWS, tuple(jobs))]


def _dense(key, max_k, a, e, why):
    return [planted_job(key, max_k, a, r, why) for r in range(e - 32, e + 32)]


@functools.lru_cache(maxsize=None)
def family_lengths_dense(max_k):
    """... and every rank of 8160 .. 8223 at a = 129 (64-bit unranking, level-3 tables, the first chunk end of a full segment)"""
    key = (MID_B, max_k, 0.0, 0.0, "")
    return [Batch("lengths_dense", key, max_k, N_ROWS, tuple(_dense(key, max_k, 129, CHUNK, "dense")))]


SHORT_A = 24
DIR_SEGLEN, DIR_SEG_TARGET = 512, 16384  # segments of 512 ranks: FW_SEG_TARGET = 16 384 for the three jobs of "deep_size4"


@functools.lru_cache(maxsize=None)
def family_level2(max_k):
    """2. level-2 cap (a = 65: exact fill, 66 and 88: the chunk ends in front of sub-block (0, 2)) and, in a short list, the directory
    limit and every size change down to the very last rank"""
    key = (MID_B, max_k, 0.0, 0.0, "")
    jobs = []
    for a in (65, 66, 88):
        if max_k == 5:
            jobs += [planted_job(key, 5, a, r, "cap a=%d" % a) for r in _around(C(a - 2, 3))]
        else:  # size 4: sub-block (0, 1) holds C(a - 2, 2) tests
            jobs += [planted_job(key, 4, a, r, "cap a=%d" % a) for r in _around(C(a - 2, 2))]
    out = [Batch("level2_cap", key, max_k, N_ROWS, tuple(jobs))]
    a = SHORT_A
    N = _job_ranks(a, MAX_TESTS, max_k)
    ranks = {N - 1}
    for s in range(max_k, 1, -1):
        e = first_rank(a, max_k, s - 1)
        ranks |= {e - 1, e}
    dirs = model_ends(a, max_k, 0, N, "l2", "dir")
    for s in (5, 4):
        inside = [e for e in dirs if size_of(e - 1, a, max_k)[0] == s and size_of(e + 1, a, max_k)[0] == s]
        for e in inside[:1] + inside[-1:]:
            ranks |= set(_around(e))
    by_size = collections.defaultdict(list)
    for r in _dedup(ranks, N):
        by_size[size_of(r, a, max_k)[0]].append(r)
    for s, rs in sorted(by_size.items(), reverse=True):
        ks = (a, s, 0.0, COLLIDE, "")  # colliding bystanders: a set smaller than max_k stops the job
        out.append(Batch("short_size%d" % s, ks, max_k, N_ROWS_COLLIDE, tuple(planted_job(ks, max_k, a, r, "short") for r in rs)))
    return out


@functools.lru_cache(maxsize=None)
def family_level2_dense(max_k):
    e = C(64, 3) if max_k == 5 else C(64, 2)
    key = (MID_B, max_k, 0.0, 0.0, "")
    return [Batch("level2_dense", key, max_k, N_ROWS, tuple(_dense(key, max_k, 66, e, "dense")))]


@functools.lru_cache(maxsize=None)
def family_level3(max_k):
    """3. level-3 cap: one sub-block (a = 451 / 452 at ranks 0 .. 2: 448 / 449 positions), two sub-blocks from rank 0 (a = 227 / 228: the
    edge of sub-block (0, 1, 2) at C(a - 3, 2), or a - 3 and 2 a - 7 at max_k 4), the first cap end of a = 228 in full segments as the
    model places it; at max_k 4 the first z1-block edge of a = 89, 128, 129, 131"""
    key = (MID_B, max_k, 0.0, 0.0, "")
    jobs = []
    for a in (227, 228):
        for e in ((C(a - 3, 2),) if max_k == 5 else (a - 3, 2 * a - 7)):
            jobs += [planted_job(key, max_k, a, r, "cap2 a=%d" % a) for r in _around(e)]
    for e in model_ends(228, max_k, CHUNK, 5 * CHUNK, "l3", "cap")[:1]:
        jobs += [planted_job(key, max_k, 228, r, "cap model") for r in _around(e)]
    for a in (451, 452):
        jobs += [planted_job(key, max_k, a, r, "cap1 a=%d" % a) for r in (0, 1, 2)]
    if max_k == 4:
        for a in (89, 128, 129, 131):
            e = C(a - 1, 3)
            jobs += [planted_job(key, 4, a, r, "z1 a=%d" % a) for r in (e - 1, e)]
    return [Batch("level3", key, max_k, N_ROWS, tuple(jobs))]


@functools.lru_cache(maxsize=None)
def family_level3_dense(max_k):
    e = C(225, 2) if max_k == 5 else 225
    key = (MID_B, max_k, 0.0, 0.0, "")
    return [Batch("level3_dense", key, max_k, N_ROWS, tuple(_dense(key, max_k, 228, e, "dense")))]


@functools.lru_cache(maxsize=None)
def family_deep():
    """3, the dear jobs: the 4 -> 3 size change of a = 89 at max_k 4 (rank C(89, 4) = 2 441 626), the last level-3 directory end in front
    of it (64 sub-blocks of a few positions each: the tail of the enumeration) and the first z1-block edge of a = 89 at max_k 5 (rank
    C(88, 4) = 2 331 890)"""
    e43 = C(89, 4)
    assert e43 == 2_441_626 and C(88, 4) == 2_331_890
    k4, k3, k5 = (89, 4, 0.0, 0.0, ""), (89, 3, 0.0, COLLIDE, ""), (89, 5, 0.0, 0.0, "")
    j4 = [planted_job(k4, 4, 89, e43 - 1, "4->3")]
    for e in model_ends(89, 4, e43 - 30000, e43, "l3", "dir", DIR_SEGLEN)[-1:]:  # (none with segments of 256 or 8 192 ranks)
        j4 += [planted_job(k4, 4, 89, r, "dir model") for r in (e - 1, e)]
    return [Batch("deep_size4", k4, 4, N_ROWS, tuple(j4)),
            Batch("deep_size3", k3, 4, N_ROWS_COLLIDE, (planted_job(k3, 4, 89, e43, "4->3"), planted_job(k3, 4, 89, e43 + 1, "4->3"))),
            Batch("deep_z1", k5, 5, N_ROWS, (planted_job(k5, 5, 89, C(88, 4) - 1, "z1"), planted_job(k5, 5, 89, C(88, 4), "z1")))]


LEAK = 0.25


@functools.lru_cache(maxsize=None)
def family_maximum():
    """4. every test significant: the maximum p sits at the planted rank and has to survive the merge across lanes, chunks, segments and
    windows.  a = 30 at max_k 5 (windows [0, 256), [256, 65 792), [65 792, N)): first window, both sides of both window edges, deep
    inside the last window, the last subset of five; a = 40 at max_k 4 (level 2) and a = 89 at max_k 4 (long lists, behind the first
    z1-block); the underflow job: every p is 0 and the last rank wins."""
    k5, k4s, k4l, ku = (30, 5, LEAK, 0.0, ""), (40, 4, LEAK, 0.0, ""), (89, 4, LEAK, 0.0, ""), (20, 5, 3.0, 0.0, "")
    w1 = W0_SMALL + W0_SMALL * 256
    r5 = (100, 255, 256, 8192, w1 - 1, w1, 100_000, C(30, 5) - 1)
    nu = _job_ranks(20, MAX_TESTS, 5)
    under = Job(20, nu - 1, tuple(range(2, 22)), "last", "underflow")
    return [Batch("max_5", k5, 5, N_ROWS, tuple(planted_job(k5, 5, 30, r, "max") for r in r5)),
            Batch("max_4_short", k4s, 4, N_ROWS, (planted_job(k4s, 4, 40, 50_000, "max"), planted_job(k4s, 4, 40, 255, "max"))),
            Batch("max_4_long", k4l, 4, N_ROWS, (planted_job(k4l, 4, 89, 1_000_000, "max"),)),
            Batch("underflow", ku, 5, 200_000, (under,))]


@functools.lru_cache(maxsize=None)
def family_maximum_dense():
    """... and every rank of 224 .. 287 of a list of 12 (1 585 subsets): both sides of the first window edge"""
    key = (12, 5, LEAK, 0.0, "")
    return [Batch("max_dense", key, 5, N_ROWS, tuple(_dense(key, 5, 12, W0_SMALL, "dense")))]


FORM_A = (40, 100, 600)   # level-2 tables, level-3 tables, the gather form


@functools.lru_cache(maxsize=None)
def family_forms(max_k):
    """5. the twin (cor = 1.0: a zero denominator, the literal 0.0; the enumeration goes on to the planted stop) in front of the planted
    set's tail -- tested together before the stop, first as the last two positions, then as (z2, z3) of the tables -- and behind it (in
    the tables of every sub-block, never tested together); the constant column (NaN) at position 30: the tests in front of its stop
    share its chunk."""
    out = []
    for a in FORM_A:
        kt, kc = (a - max_k + 1, max_k, 0.0, 0.0, "twin"), (a - max_k + 1, max_k, 0.0, 0.0, "const")
        last = 2 + max_k + kt[0] - 1          # id of the varied column; last - 1: its twin
        head = list(range(max_k - 2))         # S at (0 .. max_k - 3, l, m)
        jobs = []
        for name, tw, tail in (("front", (max_k - 2, max_k - 1), (max_k + 1, max_k + 3)), ("behind", (max_k + 4, max_k + 5), (max_k, max_k + 2))):
            pos = head + list(tail)
            placed = {q: 2 + t for t, q in enumerate(pos)}
            placed.update({tw[0]: last - 1, tw[1]: last})
            fill = [v for v in range(2 + max_k, last - 1)]
            jobs.append(Job(a, rank_of(pos, a, max_k), make_list(a, placed, fill), "stop", "twin " + name))
        if a <= 100:  # the twin as (z2, z3): S = (0, 3, 4, 5[, 6]) behind the sub-blocks of (0, 1, .) and (0, 2, .)
            pos = [0] + list(range(3, 3 + max_k - 1))
            placed = {q: 2 + t for t, q in enumerate(pos)}
            placed.update({1: last - 1, 2: last})
            jobs.append(Job(a, rank_of(pos, a, max_k), make_list(a, placed, range(2 + max_k, last - 1)), "stop", "twin z2 z3"))
            # the twin as (z2, z4): rho(z4, z2 | z1) = 1.0 is a Float64 literal in ONE position entry of the level-3 tables of sub-block
            # (0, 1, 2) -- its tests take the typed form, the others of the same chunk the NaN-free one.  S = (0, 2, 3, 5[, 6])
            pos = [0, 2, 3] + list(range(5, 5 + max_k - 3))
            placed = {q: 2 + t for t, q in enumerate(pos)}
            placed.update({1: last - 1, 4: last})
            jobs.append(Job(a, rank_of(pos, a, max_k), make_list(a, placed, range(2 + max_k, last - 1)), "stop", "twin z2 z4"))
        out.append(Batch("twin_%d" % a, kt, max_k, N_ROWS, tuple(jobs)))
        q = 30
        pos = list(range(max_k - 1)) + [q]      # the first subset that holds position q
        placed = {q: last}
        placed.update({a - max_k + t: 2 + t for t in range(max_k)})  # S at the far end: never reached
        out.append(Batch("const_%d" % a, kc, max_k, N_ROWS,
                         (Job(a, rank_of(pos, a, max_k), make_list(a, placed, range(2 + max_k, last)), "nan", "const"),)))
    return out


def families(max_k):
    """every host-pool batch of one max_k (the deep jobs and the maximum family: see all_batches)"""
    return (family_lengths(max_k) + family_lengths_dense(max_k) + family_level2(max_k) + family_level2_dense(max_k) + family_level3(max_k) +
            family_level3_dense(max_k) + family_forms(max_k))


def all_batches():
    return families(4) + families(5) + family_deep() + family_maximum() + family_maximum_dense()


def long_segment_batches():
    """6. the batches of families 2, 3 and 4 again, for the run under FW_SEG_TARGET = 1 (segments of 8 192 ranks)"""
    out = []
    for mk in (4, 5):
        out += family_level2(mk) + family_level2_dense(mk) + family_level3(mk) + family_level3_dense(mk)
    return out + family_deep() + family_maximum() + family_maximum_dense()


# ---- the oracle's side ----
@functools.lru_cache(maxsize=None)
def oracle_results(batch):
    """Oracle.test_subsets of every job of the batch (cached per process: the batches are hashable tuples)"""
    from oracle import oracle as O
    orc = O.Oracle("fz", cor_mat=table(*batch.key), n_obs=batch.n_obs)
    try:
        return tuple(orc.test_subsets(0, 1, list(j.acc), max_k=batch.max_k, alpha=ALPHA, n_obs_min=20, max_tests=MAX_TESTS) for j in batch.jobs)
    finally:
        orc.close()
