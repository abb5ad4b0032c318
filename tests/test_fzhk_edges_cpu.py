"""The tables, the model and the job lists of tests/fzhk_edges_tables.py on the CPU alone: the constants are the #defines, the extended
pool plan is the native one, every job ends on the oracle where its family says, and every switch of the model has a job on both sides
-- so no comparison of tests/test_gpu_fzhk_edges.py is vacuous.

Figures of the oracle, measured with these generators (alpha = 0.01; 4 000 rows, 40 000 for the colliding tables; one CPU core).
Per function of the GPU module: jobs by outcome, the oracle's tests (the summed stop ranks), its time, the range of the returned p.

  family         jobs                     oracle tests   time    p
  lengths  4     144 stop                   1 184 860    1.5 s   0.17 .. 0.42
  lengths  5     144 stop                   1 184 860    2.0 s   0.011 .. 0.80
  level2   4      83 stop                     269 127    0.3 s   0.04 .. 0.98
  level2   5      82 stop                   3 685 576    5.8 s   0.04 .. 0.98
  level3   4      93 stop                   2 328 759    1.4 s   0.42
  level3   5      76 stop                   1 763 378    3.0 s   0.80
  deep size 4      3 stop                   7 319 769    3.2 s   0.33
  deep size 3      2 stop                   4 883 255    2.2 s   0.996
  deep z1 (5)      2 stop                   4 663 781    6.0 s   0.76
  maximum         75 max, 1 last            4 282 002    3.2 s   0 (underflow), 1.2e-19 .. 1e-08
  forms    4      10 stop, 3 NaN               19 979    0.5 s   0.34 .. 0.57, NaN
  forms    5      10 stop, 3 NaN              480 129    0.9 s   0.38 .. 0.67, NaN

731 jobs in 41 batches, none with another outcome than its family's.  Rates: 0.8e6 tests of five variables and 2.3e6 of four per
second.  The twin (cor = 1.0) lets the enumeration go on to the planted stop in all 20 jobs; the constant column stops its job with
a NaN statistic at rank q - max_k + 1 of list position q = 30 (num_tests 28 at max_k 4, 27 at max_k 5) for 40, 100 and 600 variables.

Where the model puts the jobs (test_every_switch_of_the_model_has_a_job_on_both_sides): under the default plan chunks end by the
level-2 cap, the level-3 cap, a size change and the segment; the level-2 directory limit (96 sub-blocks) closes a chunk only in segments
of 8 192 ranks (FW_SEG_TARGET = 1), the level-3 one (64 sub-blocks) only in segments of a few hundred ranks inside a small z1-block
(FW_SEG_TARGET = 16 384 for the three deep jobs: 512 ranks); no chunk of the host pool ends by its run length -- a segment is never
longer than a chunk there -- which is what the device-rounds case of the GPU module is for.  At max_k 4-5 the long-list kernel keeps
the list in LDS up to 512 variables only, so 2 048 | 2 049 crosses no switch of its own; the lengths are kept as listed.
"""
import collections
import os
import re
import subprocess
import time

import numpy as np
import pytest

from tests import fzhk_edges_tables as TB
from tests.pool_plan import _job_ranks, _plan
from tests.util import ROOT

CSRC = os.path.join(ROOT, "flashweave.jl_amd", "csrc")
C = TB.C


def test_constants_equal_the_defines():
    rows = [ln.split() for ln in TB.DEFINES.strip().splitlines()]
    assert len(rows) == 11
    for fname, name, value in rows:
        with open(os.path.join(CSRC, fname), encoding="utf-8") as f:
            found = re.findall(r"^#define\s+%s\s+([0-9.]+)\b" % name, f.read(), re.M)
        assert found and {float(v) for v in found} == {float(value)}, (fname, name, value, found)
    assert (TB.HK_A, TB.L1_A, TB.ACC_LDS, TB.UNRANK32_A5, TB.HK_CAP, TB.HK_DIR, TB.L3_CAP, TB.L3_DIR, TB.CHUNK) == (88, 512, 2048, 128, 4096, 96, 448, 64, 8192)
    # what the issue's edges rest on: an exact fill at 65, one entry set too many at 66; 448 positions at 451; two sub-blocks at 227
    assert TB._hk_entries(63) + TB._hk_entries(62) == TB.HK_CAP < TB._hk_entries(64) + TB._hk_entries(63)
    assert 451 - 3 == TB.L3_CAP and (227 - 3) + (227 - 4) <= TB.L3_CAP < (228 - 3) + (228 - 4)
    assert (C(63, 3), C(64, 3), C(86, 3), C(88, 3), C(89, 4), C(88, 4)) == (39711, 41664, 102340, 109736, 2441626, 2331890)
    # the 32-bit products of fw_binom32 hold well past 131 (C(m, 4) (m - 4) < 2^32 up to 161); the ranks of 128 fit 32 bits
    assert C(131, 4) * 127 < 1 << 32 and C(161, 4) * 157 < 1 << 32 <= C(162, 4) * 158 and C(128, 5) < 1 << 32


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pool_check") / "pool_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", out, os.path.join(ROOT, "tests", "native", "pool_check.cpp")], check=True)
    return out


def _native_plan(exe, alens, max_k, seg_target=0, max_tests=TB.MAX_TESTS):
    tokens = ["plan", 1, seg_target, 0, 1 << 22, 16384, max_k, max_tests, len(alens), *alens]
    r = subprocess.run([exe], input=" ".join(map(str, tokens)), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    plan = []
    for ln in r.stdout.splitlines():
        v = [int(x) for x in ln.split()]
        plan.append((v[0], [tuple(v[3 + 3 * t:6 + 3 * t]) for t in range(v[2])]))
    return plan


@pytest.mark.parametrize("seg_target", [0, 1, TB.DIR_SEG_TARGET])
@pytest.mark.parametrize("max_k", [3, 4, 5])
def test_extended_pool_plan_equals_the_native_plan(exe, max_k, seg_target):
    for alens in ([24], [12, 30, 40], [63, 64, 66, 88, 89], [89, 89, 89], [131, 228, 452, 600], [20] * 40 + [100] * 3):
        ref = _plan(alens, TB.MAX_TESTS, max_k, None, seg_target)
        assert _native_plan(exe, alens, max_k, seg_target) == ref, (alens, max_k, seg_target)
        if seg_target == 1:
            assert all(s == min(8192, -(-sum(hi - lo for _, lo, hi in wins) // 256) * 256) for s, wins in ref)  # a full segment from 7 937 ranks on
    assert _job_ranks(89, TB.MAX_TESTS, 4) == 2_559_195 and _job_ranks(20, TB.MAX_TESTS, 5) == 21_699
    # a job that stops leaves after the launch whose window holds the stop; the others go on
    p = _plan([89, 89], TB.MAX_TESTS, 4, [16383, 16384], 0)
    assert [[w[0] for w in wins] for _, wins in p] == [[0, 1], [1]] and p[1][1][0][1:] == (16384, 2_559_195)


def _outcome_ok(batch, job, e):
    zs = TB.zs_of(job, batch.max_k)
    if job.expect == "stop":
        return e["status"] == 1 and e["num_tests"] == job.rank + 1 and tuple(e["Zs"]) == zs and TB.ALPHA <= e["pval"] < 1.0 and e["stat"] != 0.0
    if job.expect == "nan":
        return e["status"] == 1 and e["num_tests"] == job.rank + 1 and tuple(e["Zs"]) == zs and np.isnan(e["stat"]) and np.isnan(e["pval"])
    N = _job_ranks(job.a, TB.MAX_TESTS, batch.max_k)
    if job.expect == "max":
        return e["status"] == 2 and e["num_tests"] == N and tuple(e["Zs"]) == zs and 0.0 < e["pval"] < TB.ALPHA
    return e["status"] == 2 and e["num_tests"] == N and job.rank == N - 1 and tuple(e["Zs"]) == (job.acc[-1],) and e["pval"] == 0.0  # "last"


FAMILIES = {
    "lengths_4": lambda: TB.family_lengths(4) + TB.family_lengths_dense(4), "lengths_5": lambda: TB.family_lengths(5) + TB.family_lengths_dense(5),
    "level2_4": lambda: TB.family_level2(4) + TB.family_level2_dense(4), "level2_5": lambda: TB.family_level2(5) + TB.family_level2_dense(5),
    "level3_4": lambda: TB.family_level3(4) + TB.family_level3_dense(4), "level3_5": lambda: TB.family_level3(5) + TB.family_level3_dense(5),
    "deep_size4": lambda: TB.family_deep()[:1], "deep_size3": lambda: TB.family_deep()[1:2], "deep_z1": lambda: TB.family_deep()[2:],
    "maximum": lambda: TB.family_maximum() + TB.family_maximum_dense(),
    "forms_4": lambda: TB.family_forms(4), "forms_5": lambda: TB.family_forms(5),
}


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_every_job_ends_where_its_family_says(name):
    """status, num_tests and the conditioning set on the oracle alone: a planted job stops at its rank with alpha <= p < 1 (every
    earlier test is significant), a leaky job runs through with its maximum 0 < p < alpha at its rank, the constant column stops its job
    with a NaN statistic at the first subset that holds it, the underflow job returns p = 0 and the last variable of the list."""
    t0 = time.time()
    cnt, tests, bad, ps = collections.Counter(), 0, [], []
    for b in FAMILIES[name]():
        for job, e in zip(b.jobs, TB.oracle_results(b)):
            cnt[job.expect] += 1
            tests += e["num_tests"]
            ps.append(e["pval"])
            if not _outcome_ok(b, job, e):
                bad.append((b.name, b.max_k, job.a, job.rank, job.expect, job.why, e))
    print("%-12s %s, %d oracle tests, %.1f s, p %.2g .. %.2g" % (name, dict(cnt), tests, time.time() - t0, np.nanmin(ps), np.nanmax(ps)))
    assert not bad, (len(bad), bad[:3])
    assert tests <= 8_000_000  # a function's share of oracle time stays at a few seconds


def test_batches_are_the_same_in_every_process():
    a, b = TB.family_level2(5), TB.family_level2(5)
    assert a is b and TB.table(24, 1, 0.0, TB.COLLIDE, "") is TB.table(24, 1, 0.0, TB.COLLIDE, "")
    cm = TB.table(36, 5, 0.0, 0.0, "twin")
    assert cm.dtype == np.float32 and (cm == cm.T).all() and (np.diag(cm) == 1).all() and cm[-1, -2] == 1.0 and cm.flags.f_contiguous
    cc = TB.table(36, 5, 0.0, 0.0, "const")
    assert np.isnan(cc[-1, :-1]).all() and np.isnan(cc[:-1, -1]).all() and not np.isnan(cc[:-1, :-1]).any()
    for batch in TB.all_batches():
        p = 2 + batch.key[1] + batch.key[0]  # X, Y, S, bystanders
        for j in batch.jobs:
            assert len(j.acc) == j.a == len(set(j.acc)) and min(j.acc) >= 2 and max(j.acc) < p
        assert batch.n_obs in (TB.rows_of(batch.key), 200_000)


# (form, reason, side) the model must see under at least one of the three plans the GPU module runs
REQUIRED = {(form, reason, side) for side in ("last", "first") for form, reason in
            (("l2", "cap"), ("l2", "dir"), ("l2", "size"), ("l2", "segment"), ("l3", "cap"), ("l3", "dir"), ("l3", "segment"), ("l1", "segment"),
             ("gather", "segment"))} | {(form, "inside", "") for form in ("l2", "l3", "l1", "plain_size", "plain_z1", "gather", "inlane")}


def test_every_switch_of_the_model_has_a_job_on_both_sides():
    default = TB.coverage(TB.all_batches())
    full = TB.coverage(TB.long_segment_batches(), 1)
    short = TB.coverage(TB.family_deep()[:1], TB.DIR_SEG_TARGET)
    print("default plan:", sorted(default - {c for c in default if c[1] == "inside"}))
    print("segments of 8192 add:", sorted(full - default))
    print("segments of 512 add:", sorted(short - default - full))
    assert REQUIRED <= default | full | short, sorted(REQUIRED - (default | full | short))
    # where each plan is needed: the level-2 directory limit closes a chunk only inside long segments, the level-3 one only in short ones
    assert ("l2", "dir", "last") in full and ("l2", "dir", "last") not in default
    assert ("l3", "dir", "last") in short and ("l3", "dir", "last") not in default | full
    # the host pool never cuts a segment longer than a chunk: "run" is left to the device rounds (tests/test_gpu_fzhk_edges.py, case 7)
    assert not [c for c in default | full | short if c[1] == "run"]
    # list lengths: every routing switch with stops in the first lane, chunk, segment and window
    lens = {(j.a, j.rank) for mk in (4, 5) for b in TB.family_lengths(mk) for j in b.jobs}
    assert lens == {(a, r) for a in (88, 89, 128, 129, 130, 131, 512, 513, 2048, 2049) for r in (0, 255, 256, 8191, 8192, 16383, 16384, 16385)}


def test_model_on_hand_counted_chunks():
    """The walks against cuts counted by hand from csrc/fw_fz_core.h."""
    # a = 66, max_k 5: from rank 40 960 sub-block (0, 1) takes 2145 entries, (0, 2) 2080 more: the chunk ends at C(64, 3)
    assert TB.chunks(66, 5, 40960, 49152)[0] == TB.Chunk(40960, C(64, 3), "l2", "cap")
    # a = 65: (0, 1) and (0, 2) fill the table exactly; the segment ends first
    assert TB.chunks(65, 5, 32768, 40960) == [TB.Chunk(32768, 40960, "l2", "segment")]
    # a = 451 | 452 at rank 0: 448 | 449 positions
    assert TB.chunks(451, 5, 0, 256)[0].form == "l3" and TB.chunks(452, 5, 0, 256)[0].form == "l1"
    # a = 227 | 228, max_k 4, a segment from rank 0: two sub-blocks | one
    assert TB.chunks(227, 4, 0, 8192)[0][:2] == (0, 224 + 223) and TB.chunks(228, 4, 0, 8192)[0] == TB.Chunk(0, 225, "l3", "cap")
    # a = 89, max_k 4: a segment across the first z1-block edge leaves the tables, one across the 4 -> 3 change too
    e = C(88, 3)
    assert [c.form for c in TB.chunks(89, 4, e - 100, e + 156)] == ["plain_z1"] and [c.form for c in TB.chunks(89, 4, C(89, 4) - 6, C(89, 4) + 250)] == ["plain_size"]
    # level 2 ends a chunk at every size change; sizes 3 and below are in-lane
    ch = TB.chunks(24, 5, C(24, 5) - 100, C(24, 5) + 156)
    assert [(c.hi, c.form, c.reason) for c in ch] == [(C(24, 5), "l2", "size"), (C(24, 5) + 156, "l2", "segment")]
    assert TB.chunks(24, 5, C(24, 5) + C(24, 4), C(24, 5) + C(24, 4) + 256)[0].form == "inlane" and TB.chunks(600, 5, 0, 8192)[0].form == "gather"
    # unranking and ranking are inverse
    for a, mk in ((24, 5), (89, 4)):
        for r in (0, 1, 255, C(a, mk) - 1, C(a, mk), _job_ranks(a, TB.MAX_TESTS, mk) - 1):
            assert TB.rank_of(TB.unrank(r, a, mk), a, mk) == r
