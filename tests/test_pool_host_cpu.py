"""csrc/fw_pool_host.h -- the host job pool's pure rules (enumeration size, first window, segment length, growth, cut, merge, advance,
unranking) -- compiled natively through tests/native/pool_check.cpp: no GPU, no build of the library.

The plan is compared with tests/pool_plan.py (the restatement tests/test_gpu_fz_screen.py plans its batches with), merge and advance with a
sequential Python reference on hand-made record sequences.  Doubles cross the text boundary as the hex digits of their bits."""
import itertools
import math
import os
import struct
import subprocess

import pytest

from tests.pool_plan import _job_ranks, _plan
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "pool_check.cpp")
HEADER = os.path.join(ROOT, "flashweave.jl_amd", "csrc", "fw_pool_host.h")
SAT = 1 << 62
STOPPED, ALL_SIG = 1, 2  # FW_SUBSETS_*


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _hex(x):
    return "%016x" % _bits(x)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pool_check") / "pool_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", out, SRC], check=True)
    return out


def _run(exe, tokens):
    r = subprocess.run([exe], input=" ".join(map(str, tokens)), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.splitlines()


def test_header_compiles_without_hip(tmp_path):
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "%s"\nint main() { return 0; }\n' % HEADER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-H", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    included = [ln for ln in r.stderr.splitlines() if ln.startswith(".")]  # -H: one line per header, dots for the depth
    assert included and not [ln for ln in included if "hip" in ln.lower()]


# ---- 1. enumeration size ----
def _enum_ref(a, max_k, max_tests):
    N = min(sum(math.comb(a, s) for s in range(1, max_k + 1)), SAT)
    return min(N, max_tests) if max_tests > 0 else N


def test_enumeration_size_equals_math_comb(exe):
    cases = []
    for max_k in range(1, 8):
        for a in sorted({0, 1, max_k - 1, max_k, 63, 64, 512, 513}):
            for max_tests in (0, 10_000_000, 5):
                cases.append((a, max_k, max_tests))
    assert all(math.comb(a, s) <= 2 * 10**18 for a, k, _ in cases for s in range(1, k + 1))  # nothing here saturates: exact sums
    got = [int(x) for x in _run(exe, ["enum", len(cases), *itertools.chain.from_iterable(cases)])]
    assert got == [_enum_ref(*c) for c in cases]
    assert _enum_ref(513, 7, 0) > 10**15 and _enum_ref(0, 3, 0) == 0 and _enum_ref(2, 3, 0) == 3
    # C(100 000, 5) = 8.3e22 saturates; the cap still applies
    assert math.comb(100_000, 5) > SAT
    assert [int(x) for x in _run(exe, ["enum", 2, 100_000, 5, 0, 100_000, 5, 10_000_000])] == [SAT, 10_000_000]


def test_unranking_walks_sizes_max_k_to_1_in_lexicographic_order(exe):
    for a, max_k in ((9, 7), (7, 7), (12, 3), (1, 3), (5, 6)):
        exp = [list(c) for s in range(max_k, 0, -1) for c in itertools.combinations(range(a), s)]
        out = _run(exe, ["unrank", a, max_k, len(exp), *range(len(exp))])
        got = [[int(x) for x in ln.split()] for ln in out]
        assert [g[0] for g in got] == [len(e) for e in exp] and [g[1:] for g in got] == exp, (a, max_k)


# ---- 2. the plan ----
def _native_plan(exe, alens, fz=1, seg_target=0, forced=0, small=1 << 22, w0_big=16384, max_k=3, max_tests=10_000_000):
    out = _run(exe, ["plan", fz, seg_target, forced, small, w0_big, max_k, max_tests, len(alens), *alens])
    plan = []
    for ln in out:
        v = [int(x) for x in ln.split()]
        seglen, ns, nwin = v[:3]
        wins = [tuple(v[3 + 3 * t:6 + 3 * t]) for t in range(nwin)]
        assert ns == sum(-(-(hi - lo) // seglen) for _, lo, hi in wins)
        plan.append((seglen, wins))
    return plan


@pytest.mark.parametrize("name,alens", [("one_small", [3]), ("w0_switch", [63, 64]), ("table_switch", [512, 513]), ("many_of_5", [5] * 3000),
                                        ("past_small_launch", [100] * 300 + [48] * 10)])
def test_plan_equals_the_python_restatement(exe, name, alens):
    ref = _plan(alens)
    assert _native_plan(exe, alens) == ref
    totals = [sum(hi - lo for _, lo, hi in wins) for _, wins in ref]
    if name == "w0_switch":
        assert [hi for _, _, hi in ref[0][1]] == [256, 16384]
    if name == "table_switch":  # capped by max_tests: 16 384, then x256 twice; last launch: ceil256(2 * 5 789 312 // 3 072 = 3 769)
        assert [w[0][2] for _, w in ref] == [16384, 16384 * 257, 10_000_000] and ref[-1][0] == 3840
    if name == "past_small_launch":  # the first launch passes 1 << 22 ranks: x16, not x256, and segments longer than one workgroup's 256
        assert totals[0] >= 1 << 22 and ref[0][0] == 1792 and ref[1][1][-1][2] - ref[1][1][-1][1] == 16 * 256
        assert totals[1] > 3072 * 8192 and ref[1][0] == 8192  # the longest segment there is


def test_growth_by_launch_size_live_jobs_and_the_forced_factor(exe):
    # 3 000 jobs of 5 need one round; what the next round would have been is the width the advance leaves: checked through jobs of 40
    # accepted variables (10 700 ranks: 256, then the rest) with the small-launch bound lowered so that the job count decides
    many, few = [40] * 3000, [40] * 100
    for alens, growth in ((many, 4), (few, 16)):
        plan = _native_plan(exe, alens, small=1)
        assert plan[0][1][0][1:] == (0, 256) and plan[1][1][0][1:] == (256, 256 + 256 * growth), growth
    assert _native_plan(exe, few)[1][1][0][1:] == (256, _job_ranks(40))  # default bound: a small launch, x256
    assert _native_plan(exe, few, forced=7)[1][1][0][1:] == (256, 256 + 256 * 7)
    assert _native_plan(exe, many, small=1, forced=2)[1][1][0][1:] == (256, 256 + 512)


def test_discrete_constants_and_the_segment_target(exe):
    # discrete: first window 16, 4-rank granularity, segments of 8..256 ranks, 4 096 workgroups aimed for
    plan = _native_plan(exe, [20] * 5000, fz=0)
    assert [hi - lo for _, lo, hi in plan[0][1]] == [16] * 5000 and plan[0][0] == 20  # ceil4(80 000 / 4 096 = 19)
    assert _native_plan(exe, [20], fz=0)[0][0] == 8 and _native_plan(exe, [30] * 5000, fz=0, small=1, forced=64)[1][0] == 256
    # fz: 256..8 192 in steps of 256, 3 072 aimed for; a target of its own replaces it
    assert _native_plan(exe, [100] * 300)[0][0] == 1792 and _native_plan(exe, [100] * 300, seg_target=16384)[0][0] == 512
    assert _native_plan(exe, [64], w0_big=512)[0][1] == [(0, 0, 512)]


def test_cut_tiles_the_window(exe):
    for lo, hi, seglen in ((0, 256, 256), (0, 257, 256), (16384, 16384 + 5000, 1792), (7, 8, 8192), (5, 5, 256)):
        segs = [tuple(int(x) for x in ln.split()) for ln in _run(exe, ["cut", lo, hi, seglen])]
        exp = [(s, min(hi, s + seglen)) for s in range(lo, hi, seglen)]
        assert segs == exp and len(segs) == -(-(hi - lo) // seglen)


# ---- 3. merge and advance ----
def _seg(stop=None, best=None, evaluated=0):
    """stop = (rank, stat, pval, df, power), best = (rank, stat, pval, df)"""
    s = stop or ("none", 0.0, 0.0, 0, 0)
    b = best or (0, 0.0, -1.0, 0)
    return dict(stop_rank=s[0], stop_stat=s[1], stop_pval=s[2], stop_df=s[3], stop_power=s[4], best_rank=b[0], best_stat=b[1], best_pval=b[2],
                best_df=b[3], evaluated=evaluated)


def _reference(N, nxt, width, cmds):
    """fw_pool_merge / fw_pool_advance, sequentially"""
    j = dict(done=0, no_zs=0, next=nxt, width=width, best_rank=0, best_df=0, best_p=-1.0, best_stat=0.0, stat=0.0, pval=0.0, num_tests=0,
             evaluated=0, df=0, suff_power=0, status=0)
    for c in cmds:
        if isinstance(c, dict):
            j["evaluated"] += c["evaluated"]
            if j["done"]:
                continue
            if c["stop_rank"] != "none":
                j.update(stat=c["stop_stat"], pval=c["stop_pval"], df=c["stop_df"], suff_power=c["stop_power"], status=STOPPED,
                         num_tests=c["stop_rank"] + 1, best_rank=c["stop_rank"], done=1)
                if c["stop_df"] == -2:
                    j.update(df=0, num_tests=0, no_zs=1)
            elif c["best_pval"] >= j["best_p"]:  # (False for NaN)
                j.update(best_p=c["best_pval"], best_stat=c["best_stat"], best_rank=c["best_rank"], best_df=c["best_df"])
        elif not j["done"]:
            j["next"] += min(j["width"], N - j["next"])
            j["width"] = (j["width"] * c) % (1 << 64)
            if j["next"] >= N:
                j.update(stat=j["best_stat"], pval=0.0 if j["best_p"] < 0.0 else j["best_p"], df=j["best_df"], suff_power=1, status=ALL_SIG,
                         num_tests=N, done=1)
    return "%d %d %d %d %d %d %s %s | %s %s %d %d %d %d %d" % (j["done"], j["no_zs"], j["next"], j["width"], j["best_rank"], j["best_df"],
                                                             _hex(j["best_p"]), _hex(j["best_stat"]), _hex(j["stat"]), _hex(j["pval"]),
                                                             j["num_tests"], j["evaluated"], j["df"], j["suff_power"], j["status"])


def _native(exe, N, nxt, width, cmds):
    tok = ["merge", N, nxt, width]
    for c in cmds:
        if isinstance(c, dict):
            tok += ["seg", c["stop_rank"], _hex(c["stop_stat"]), _hex(c["stop_pval"]), c["best_rank"], _hex(c["best_stat"]), _hex(c["best_pval"]),
                    c["stop_df"], c["stop_power"], c["best_df"], c["evaluated"]]
        else:
            tok += ["adv", c]
    return _run(exe, tok)[0]


NAN = float("nan")
MERGE_CASES = {
    # name: (N, next, width, commands, the fields that make the case: checked on the reference before the comparison)
    "stop_in_segment_0": (1000, 0, 256, [_seg(stop=(3, 1.5, 0.2, 1, 1), evaluated=256), 16], dict(done=1, status=STOPPED, num_tests=4, evaluated=256, next=0)),
    "stop_behind_speculation": (10**6, 256, 1024, [_seg(best=(300, 2.0, 0.001, 1), evaluated=256), _seg(stop=(700, 0.5, 0.6, 2, 1), evaluated=200),
                                                   _seg(best=(900, 9.0, 0.9, 1), evaluated=256), _seg(stop=(1100, 0.1, 0.9, 1, 0), evaluated=256), 4],
                                dict(done=1, status=STOPPED, num_tests=701, evaluated=968, pval=0.6, df=2, best_rank=700)),
    "equal_best_later_wins": (10**6, 0, 512, [_seg(best=(10, 1.0, 0.004, 1), evaluated=256), _seg(best=(400, -1.0, 0.004, 3), evaluated=256), 4],
                              dict(done=0, best_rank=400, best_df=3, next=512, width=2048)),
    "nan_best_never_taken": (10**6, 0, 512, [_seg(best=(10, 1.0, 0.004, 1), evaluated=256), _seg(best=(400, NAN, NAN, 3), evaluated=256), 4],
                             dict(done=0, best_rank=10, best_df=1)),
    "nan_first_then_a_value": (10**6, 0, 512, [_seg(best=(10, NAN, NAN, 1), evaluated=256), _seg(best=(400, 2.0, 0.0, 3), evaluated=256), 4],
                               dict(done=0, best_rank=400)),
    "no_test_marker": (500, 0, 256, [_seg(stop=(0, 0.0, 1.0, -2, 0), evaluated=0), _seg(best=(300, 1.0, 0.5, 1), evaluated=7), 256],
                       dict(done=1, no_zs=1, status=STOPPED, num_tests=0, df=0, evaluated=7)),
    "exhausted_with_a_best": (300, 0, 256, [_seg(best=(17, 3.0, 0.002, 1), evaluated=256), 256, _seg(best=(299, 4.0, 0.003, 2), evaluated=44), 256],
                              dict(done=1, status=ALL_SIG, num_tests=300, pval=0.003, df=2, suff_power=1, evaluated=300, next=300, best_rank=299)),
    "exhausted_without_any_best": (40, 0, 256, [_seg(best=(0, NAN, NAN, 0), evaluated=40), 16], dict(done=1, status=ALL_SIG, num_tests=40, pval=0.0, stat=0.0)),
    "window_width_wraps_like_uint64": (1 << 62, 0, 1 << 60, [256], dict(done=0, next=1 << 60, width=0)),
}
FIELDS = ["done", "no_zs", "next", "width", "best_rank", "best_df", "best_p", "best_stat", "|", "stat", "pval", "num_tests", "evaluated", "df", "suff_power", "status"]


@pytest.mark.parametrize("name", sorted(MERGE_CASES))
def test_merge_and_advance_equal_the_sequential_reference(exe, name):
    N, nxt, width, cmds, marks = MERGE_CASES[name]
    ref = _reference(N, nxt, width, cmds)
    by_name = dict(zip(FIELDS, ref.split()))
    for k, v in marks.items():
        assert by_name[k] == (_hex(v) if isinstance(v, float) else str(v)), (k, v, ref)
    assert _native(exe, N, nxt, width, cmds) == ref


# ---- 4. one binomial on the host ----
def test_shared_binomials_equal_the_long_double_form(exe):
    """fw_pool_binom (fw_binom_u64 up to t = 5, fw_binom_any for 6 and 7: double estimates) against a long-double form with the
    same bounds (tests/native/pool_check.cpp): every m up to 65 536 and 4 096 values of m on either side of the first saturating m, t = 0..7."""
    rows = [[int(x) for x in ln.split()] for ln in _run(exe, ["binom"])]
    assert [r[0] for r in rows] == list(range(8))
    assert [r[2] for r in rows] == [0] * 8, rows
    first = {r[0]: r[1] for r in rows}
    assert first[0] == first[1] == first[2] == -1  # no saturating m below 2^31
    for t in range(3, 8):
        lim = 2.0e18 if t > 5 else 3.6e18
        assert math.comb(first[t] - 1, t) <= lim < math.comb(first[t], t)
