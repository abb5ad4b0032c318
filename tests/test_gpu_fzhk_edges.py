"""The max_k 4-5 Fisher-z segment kernels (csrc/fw_fz_core.h: fz_seg_body<HIGHK, ., .> -- level-2 tables up to 88 accepted variables,
level-1 plus level-3 position tables up to 512, the gather form beyond) on and next to every point where the list length, a table
limit, a chunk, segment or window end or the arithmetic form switches the code path, against the CPU oracle, through
Engine.test_subsets_batch on a matrix given with set_cor_mat.  tests/fzhk_edges_tables.py builds the tables and job lists and models
where each job sits; tests/test_fzhk_edges_cpu.py asserts on the oracle alone that every job ends where its family says and that each
switch has a job on both sides.

Rules of comparison, those of tests/test_gpu_fz.py: status, num_tests and the conditioning set are equal, the statistic is bit-equal,
p and frac agree to 1e-12 relative, NaN results are NaN on both sides.  Every job of every batch is compared."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import flashweave_jl_amd as fw
from tests import fzhk_edges_tables as TB
from tests.util import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "fzhk_edges_worker.py")
WORKER_KNOBS = ("FW_SEG_TARGET", "FW_DH_LOG", "FW_HOST_HITON", "FW_NO_HK", "FW_FZ_DBG", "FW_W0_BIG", "FW_SMALL_LAUNCH", "FW_WINDOW_GROWTH")


def engine_results(batch):
    """The batch through Engine.test_subsets_batch, in plain dicts (the worker prints them as JSON)."""
    cm = TB.table(*batch.key)
    eng = fw.Engine("fz", batch.n_obs, cm.shape[0], max_k=batch.max_k, alpha=TB.ALPHA, max_tests=TB.MAX_TESTS)
    try:
        eng.set_cor_mat(cm)
        n = len(batch.jobs)
        got = eng.test_subsets_batch([0] * n, [1] * n, [list(j.acc) for j in batch.jobs])
    finally:
        eng.close()
    return [dict(g, Zs=[int(v) for v in g["Zs"]]) for g in got]


def _same(a, b):
    return a == b or (np.isnan(a) and np.isnan(b))


def check(batch, got, what=""):
    """Every job of the batch against the oracle; collects every miss, then asserts."""
    exp = TB.oracle_results(batch)
    assert len(got) == len(exp) == len(batch.jobs)
    bad = []
    for job, g, e in zip(batch.jobs, got, exp):
        ok = (g["status"], g["num_tests"], tuple(g["Zs"])) == (e["status"], e["num_tests"], tuple(e["Zs"]))
        ok = ok and _same(g["stat"], e["stat"])
        ok = ok and ((np.isnan(g["pval"]) and np.isnan(e["pval"])) or rel(g["pval"], e["pval"]) < 1e-12)
        ok = ok and rel(g["frac"], e["frac"]) < 1e-12 and g["suff_power"] == e["suff_power"]
        if not ok:
            bad.append((job.a, job.rank, job.why, g, e))
    print(what, batch.name, "max_k", batch.max_k, "%d jobs, %d misses" % (len(exp), len(bad)))
    assert not bad, (what, batch.name, batch.max_k, len(bad), bad[:3])


def _run(batches, what=""):
    for b in batches:
        check(b, engine_results(b), what)


# ---- 1. list-length switches ----
@pytest.mark.parametrize("max_k", [4, 5])
def test_list_length_switches(max_k):
    """|accepted| = 88 | 89 (level-2 table kernel, long-list kernel), 128 | 129, 130 | 131 (32-bit unranking of positions 4 and 5),
    512 | 513 (tables, gather form), 2048 | 2049 (list in LDS, in global memory): planted stops at ranks 0, 255 | 256, 8191 | 8192,
    16 383 | 16 384 | 16 385 -- both sides of the first lane, chunk, segment and window ends -- and every rank of 8160 .. 8223 at
    |accepted| = 129."""
    _run(TB.family_lengths(max_k) + TB.family_lengths_dense(max_k))


# ---- 2. level-2 cap and directory ----
@pytest.mark.parametrize("max_k", [4, 5])
def test_level2_cap_directory_and_size_changes(max_k):
    """FZ_HK_CAP: |accepted| = 65 (sub-blocks (0, 1) and (0, 2) fill the 4096 entries exactly), 66 and 88 (the chunk ends in front of
    (0, 2)) at the edge of sub-block (0, 1) +- 1, every rank of 64 around it at 66; a list of 24: the last subset of each size and the
    first of the next down to the very last rank, and the chunk ends by FZ_HK_DIR (tests/fzhk_edges_tables.py: model_ends)."""
    _run(TB.family_level2(max_k) + TB.family_level2_dense(max_k))


# ---- 3. level-3 cap, z1-blocks ----
@pytest.mark.parametrize("max_k", [4, 5])
def test_level3_cap_and_z1_blocks(max_k):
    """FZ_L3_CAP: |accepted| = 451 | 452 at ranks 0 .. 2 (one sub-block of 448 | 449 positions: level-3 tables | level-1 form), 227 |
    228 at the edge of sub-block (0, 1, 2), the first cap end of 228 in full segments, every rank of 64 around the edge at 228; at
    max_k 4 the last rank of z1-block 0 and the first of block 1 for 89, 128, 129, 131."""
    _run(TB.family_level3(max_k) + TB.family_level3_dense(max_k))


@pytest.mark.parametrize("index", [0, 1, 2], ids=["size4", "size3", "z1_max_k5"])
def test_deep_edges_of_89(index):
    """|accepted| = 89: the last subset of four (rank 2 441 625) and both sides of the last level-3 directory end in front of it; the
    first two subsets of three; at max_k 5 both sides of the first z1-block edge (rank 2 331 890)."""
    _run(TB.family_deep()[index:index + 1])


# ---- 4. the maximum across chunks, segments and windows ----
def test_maximum_across_chunks_segments_windows():
    """Every test significant: the planted maximum p in the first window, on both sides of both window edges, deep in the last
    window, at the last subset of five; on the level-2 form at max_k 4, on the long-list form behind the first z1-block; every rank
    of 224 .. 287 of a list of 12; the underflow job (every p is 0: the last rank wins)."""
    batches = TB.family_maximum() + TB.family_maximum_dense()
    _run(batches)
    under = [b for b in batches if b.name == "underflow"][0]
    e = TB.oracle_results(under)[0]
    assert e["pval"] == 0.0 and e["status"] == 2 and tuple(e["Zs"]) == (under.jobs[0].acc[-1],)


# ---- 5. arithmetic forms ----
@pytest.mark.parametrize("max_k", [4, 5])
def test_twin_and_constant_columns(max_k):
    """cor = 1.0 (a zero denominator: the literal 0.0) and a NaN row, per test and per table entry, on |accepted| = 40 (level-2
    tables), 100 (level-3 tables) and 600 (gather form): the twin as the last two positions, behind the planted set, as (z2, z3) and
    as (z2, z4) -- one unclean position entry among clean ones; the constant column at position 30."""
    _run(TB.family_forms(max_k))


# ---- 6. long segments: knobs the library reads once per process ----
def worker_batches(which):
    return TB.long_segment_batches() if which == "long" else TB.family_deep()[:1]


def run_worker(mode, which="long", timeout=300, **knobs):
    env = {k: v for k, v in os.environ.items() if k not in WORKER_KNOBS}
    env.update({k: str(v) for k, v in knobs.items()})
    r = subprocess.run([sys.executable, WORKER, "--mode", mode, "--which", which], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       universal_newlines=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_long_segments():
    """FW_SEG_TARGET = 1: the host pool cuts segments of 8 192 ranks, so the level-2 and level-3 directory walks of families 2, 3 and 4
    run inside full-length segments (where the cap and the directory, not the segment end, close a chunk)."""
    out = run_worker("batches", "long", FW_SEG_TARGET=1)
    batches = worker_batches("long")
    assert sorted(out, key=int) == [str(i) for i in range(len(batches))]
    for i, b in enumerate(batches):
        check(b, out[str(i)], "segments of 8192")


def test_level3_directory_limit_in_segments_of_512():
    """FZ_L3_DIR is only reached where a segment of a few hundred ranks lies inside one small z1-block: the three deep jobs of |accepted| =
    89 at max_k 4 again, cut into segments of 512 ranks (FW_SEG_TARGET = 16 384)."""
    b = worker_batches("dir")[0]
    check(b, run_worker("batches", "dir", FW_SEG_TARGET=TB.DIR_SEG_TARGET)["0"], "segments of 512")


# ---- 7. device rounds with segments longer than a chunk ----
def _two_factor():
    rng = np.random.default_rng(77)
    n, p = 2000, 260
    f = rng.standard_normal((n, 2))
    return np.asfortranarray((f[:, np.arange(p) % 2] + 2.0 * rng.standard_normal((n, p))).astype(np.float32))


def rounds_result():
    """The max_k 5 network of the two-factor table of tests/test_gpu_fz.py (lists grow to 130 variables), in plain lists."""
    data = _two_factor()
    eng = fw.Engine("fz", data.shape[0], data.shape[1], max_k=5, alpha=0.05, max_tests=60_000)
    try:
        eng.set_data(data)
        eng.cor()
        net = eng.lgl(feed_forward=True, round_size=128)
        cnt = eng.counters()
    finally:
        eng.close()
    out = {k: [float(v) for v in net[k]] for k in ("pc_off", "pc_idx", "pc_weight", "pc_pval")}
    out["edges"] = sorted([int(i), int(j), float(w)] for (i, j), w in net["edges"].items())
    out["cond_tests_ref"] = int(cnt["cond_tests_ref"])
    out["subsets_launches"] = int(cnt["subsets_launches"])
    return out


def test_device_rounds_with_segments_longer_than_a_chunk(tmp_path, monkeypatch):
    """Device rounds at max_k 5 under FW_SEG_TARGET = 64: a job's window is one segment of up to 60 000 ranks, so a workgroup walks several
    chunks of one segment (the reuse of the previous chunk's first level-2 table, the striding routing by list length, the target's
    local matrix).  Equal to the host-pool run (FW_HOST_HITON = 1, default plan) bit for bit; the log proves the long segments."""
    log = tmp_path / "dh.log"
    dev = run_worker("rounds", FW_SEG_TARGET=64, FW_DH_LOG=str(log))
    assert "FW_SEG_TARGET" not in os.environ
    monkeypatch.setenv("FW_HOST_HITON", "1")
    host = rounds_result()
    assert len(host["edges"]) > 200 and host["cond_tests_ref"] > 50_000_000 and int(max(np.diff(host["pc_off"]))) > TB.HK_A
    for key in ("edges", "pc_off", "pc_idx", "cond_tests_ref"):
        assert dev[key] == host[key], key
    for key in ("pc_weight", "pc_pval"):
        assert np.array_equal(np.array(dev[key]), np.array(host[key]), equal_nan=True), key
    rows = [[float(v) for v in ln.split()] for ln in log.read_text().splitlines() if ln and not ln.startswith("#")]
    longest = max((r[1] / r[3] for r in rows if r[3] > 0), default=0.0)  # ranks per segment of a launch, on average
    print("launches %d, longest mean segment %.0f ranks" % (len(rows), longest))
    assert longest > TB.CHUNK, longest
