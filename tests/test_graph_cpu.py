"""csrc/fw_graph.h -- the host-only part of fw_learn_network (target order, rounds, deal to ranks, running graph, make_weights,
make_symmetric_graph, FwHostWorkers) -- compiled natively through tests/native/graph_check.cpp: no GPU, no build of the library.

Doubles cross the text boundary as the hex digits of their bits, and weights are compared as bits (NaN, -0.0 included)."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import hiton_exact_ref as HR
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "graph_check.cpp")
SCHEDULES = [(True, 1), (True, 16), (False, 1)]
KINDS = ["fz", "fz_nz", "mi", "mi_nz"]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _hex(x):
    return "%016x" % _bits(x)


def _compile(tmp_path_factory, name, extra=()):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", *extra, "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(tmp_path_factory, "graph_check")


@pytest.fixture(scope="module")
def oracles():
    return HR.make_oracles()


def _run(exe, text, env=None):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout


def _graph_input(p, discrete, l0, entries, blocks):
    """l0 = (off, idx, stat); entries = [(t, u, s, pval)]; blocks = [(n_blocks, repetitions)]"""
    off, idx, stat = l0
    tok = ["graph", p, int(discrete), len(idx), *map(int, off), *map(int, idx), *map(_hex, stat), len(entries)]
    for t, u, s, pv in entries:
        tok += [int(t), int(u), _hex(s), _hex(pv)]
    tok.append(len(blocks))
    for b, r in blocks:
        tok += [b, r]
    return " ".join(map(str, tok))


def _graph_runs(out):
    """{(blocks, rep): dict of the seven arrays} with weights as bit patterns; raw: the seven lines as text"""
    lines = out.split("\n")
    runs = {}
    i = 0
    while i < len(lines) and lines[i].startswith("run "):
        _, b, r = lines[i].split()
        a = lines[i + 1:i + 8]
        runs[(int(b), int(r))] = dict(
            pc_off=[int(x) for x in a[0].split()], pc_idx=[int(x) for x in a[1].split()], pc_w=[int(x, 16) for x in a[2].split()],
            pc_p=[int(x, 16) for x in a[3].split()], e_src=[int(x) for x in a[4].split()], e_dst=[int(x) for x in a[5].split()],
            e_w=[int(x, 16) for x in a[6].split()], raw="\n".join(a))
        i += 8
    return runs


def _reference(p, discrete, l0, entries):
    """The passes in a few lines of Python on hiton_exact_ref._maxweight: stable CSR over targets, make_weights, then the edges of a
    in ascending a: outgoing entries in PC order, then incoming-only entries ascending in b; NaN edges dropped."""
    off, idx, stat = l0
    PCs = [[] for _ in range(p)]
    for t, u, s, pv in entries:
        PCs[t].append([u, s, pv])
    if discrete:
        for T in range(p):
            us = {int(idx[i]): float(stat[i]) for i in range(off[T], off[T + 1])}
            for e in PCs[T]:
                u_ = us.get(e[0], math.nan)
                sg = math.nan if math.isnan(u_) else float((u_ > 0) - (u_ < 0))
                e[1] = sg * abs(e[1])
    W = [{u: w for u, w, _ in pc} for pc in PCs]
    edges = []
    for a in range(p):
        for b, w, _ in PCs[a]:
            if b > a:
                edges.append((a, b, HR._maxweight(w, W[b].get(a, math.nan))))
        for b in range(a + 1, p):
            if a in W[b] and b not in W[a]:
                edges.append((a, b, HR._maxweight(W[b][a], math.nan)))
    edges = [e for e in edges if not math.isnan(e[2])]
    pc_off = [0]
    for pc in PCs:
        pc_off.append(pc_off[-1] + len(pc))
    return dict(pc_off=pc_off, pc_idx=[e[0] for pc in PCs for e in pc], pc_w=[_bits(e[1]) for pc in PCs for e in pc],
                pc_p=[_bits(e[2]) for pc in PCs for e in pc], e_src=[e[0] for e in edges], e_dst=[e[1] for e in edges],
                e_w=[_bits(e[2]) for e in edges])


def _same(got, exp):
    for k in ("pc_off", "pc_idx", "pc_w", "pc_p", "e_src", "e_dst", "e_w"):
        assert got[k] == exp[k], k


# ---- 1. anchored on the oracle ----
@pytest.mark.parametrize("ff,R", SCHEDULES)
@pytest.mark.parametrize("kind", KINDS)
def test_symmetric_graph_and_signs_equal_the_oracle(exe, oracles, kind, ff, R):
    orc, discrete, _ = oracles[kind]
    p = orc.p
    exp = orc.learn(max_k=3, feed_forward=ff, round_size=R)
    nb = orc.level0(alpha=0.01, hps=5, n_obs_min=orc.auto_n_obs_min(-1, 5, 3), FDR=True)
    off, idx, w, pv = exp["pc_off"], exp["pc_idx"], exp["pc_weight"], exp["pc_pval"]
    entries = [(T, int(idx[i]), float(w[i]), float(pv[i])) for T in range(p) for i in range(off[T], off[T + 1])]
    # the classes this case must contain: both directions, one direction only, NaN on one side (whitelisted entries of feed-forward)
    D = {(t, u): s for t, u, s, _ in entries}
    both = sum(1 for (t, u) in D if t < u and (u, t) in D)
    one_way = sum(1 for (t, u) in D if (u, t) not in D)
    nan_one_side = sum(1 for (t, u), s in D.items() if math.isnan(s) and not math.isnan(D.get((u, t), 0.0)))
    print("%s ff %d R %d: %d entries, %d both-direction pairs, %d one-way entries, %d NaN on one side" % (kind, ff, R, len(D), both, one_way, nan_one_side))
    assert both > 0 and one_way > 0
    if ff:
        assert nan_one_side > 0
    got = _graph_runs(_run(exe, _graph_input(p, discrete, (nb["off"], nb["idx"], nb["stat"]), entries, [(1, 1)])))[(1, 0)]
    # the directed CSR is the oracle's, and the sign pass leaves the (already signed) weights bit-equal
    assert got["pc_off"] == [int(x) for x in off] and got["pc_idx"] == [int(x) for x in idx]
    assert got["pc_w"] == [_bits(x) for x in w] and got["pc_p"] == [_bits(x) for x in pv]
    # the edges are the oracle's: the same keys, bit-equal weights ...
    keys = list(zip(got["e_src"], got["e_dst"]))
    assert len(set(keys)) == len(keys) and set(keys) == set(exp["edges"])
    assert got["e_w"] == [_bits(exp["edges"][k]) for k in keys]
    # ... in the library's order
    ref = _reference(p, False, (nb["off"], nb["idx"], nb["stat"]), entries)
    assert keys == list(zip(ref["e_src"], ref["e_dst"])) and got["e_w"] == ref["e_w"]
    assert got["e_src"] == sorted(got["e_src"])


# ---- 2. classes the oracle tables do not contain ----
def _random_case(rng, p, n_missing=3):
    """Directed lists with opposite signs, NaN on both sides, zero weights, variables without entries and neighbours that are
    missing from the level-0 list -> (level-0 CSR, entries, counts of those classes)."""
    full = [sorted(int(x) for x in rng.choice([v for v in range(p) if v != T], size=min(p - 1, int(rng.integers(0, 24))), replace=False))
            if p > 1 and rng.random() > 0.15 else [] for T in range(p)]
    entries = []
    for T in range(p):
        for u in rng.permutation(full[T]):  # PC insertion order is not ascending
            r = rng.random()
            s = math.nan if r < 0.2 else 0.0 if r < 0.3 else -0.0 if r < 0.35 else float(rng.standard_normal())
            entries.append((T, int(u), s, float(rng.random())))
    D = {(t, u): s for t, u, s, _ in entries}
    # level-0 lists: the PC neighbours (minus a few: sign NaN) plus others, statistics of either sign and zero
    off, idx, stat = [0], [], []
    missing = 0
    for T in range(p):
        nbrs = set(full[T]) | set(int(x) for x in rng.choice(p, size=min(p, 3), replace=False) if x != T)
        for u in sorted(nbrs):
            if u in full[T] and missing < n_missing and rng.random() < 0.2:
                missing += 1
                continue
            idx.append(u)
            r = rng.random()
            stat.append(0.0 if r < 0.1 else float(rng.standard_normal()))
        off.append(len(idx))
    classes = dict(
        opposite=sum(1 for (t, u), s in D.items() if t < u and (u, t) in D and s * D[(u, t)] < 0),
        nan_both=sum(1 for (t, u), s in D.items() if t < u and (u, t) in D and math.isnan(s) and math.isnan(D[(u, t)])),
        zero=sum(1 for s in D.values() if s == 0.0), empty=sum(1 for l in full if not l), missing=missing)
    return (off, idx, stat), entries, classes


@pytest.mark.parametrize("discrete", [False, True])
def test_passes_equal_python_on_random_lists(exe, discrete):
    seen = dict(opposite=0, nan_both=0, zero=0, empty=0, missing=0)
    for seed, p in enumerate([1, 2, 2, 5, 17, 40, 40, 64]):
        rng = np.random.default_rng(100 + seed)
        l0, entries, classes = _random_case(rng, p)
        for k, v in classes.items():
            seen[k] += v
        got = _graph_runs(_run(exe, _graph_input(p, discrete, l0, entries, [(1, 1), (3, 1)])))
        ref = _reference(p, discrete, l0, entries)
        _same(got[(1, 0)], ref)
        _same(got[(3, 0)], ref)
    assert all(v > 0 for v in seen.values()), seen


def test_maxweight_rules_by_hand(exe):
    # opposite signs: the lower-index endpoint's direction wins; NaN on both sides: dropped; one-way NaN: dropped; zero against a sign
    entries = [(0, 1, 2.0, 0.0), (1, 0, -3.0, 0.0), (0, 2, math.nan, 0.0), (2, 0, math.nan, 0.0), (3, 1, math.nan, 0.0),
               (2, 3, 0.0, 0.0), (3, 2, -5.0, 0.0), (4, 0, 1.5, 0.0)]
    got = _graph_runs(_run(exe, _graph_input(6, False, ([0] * 7, [], []), entries, [(1, 1)])))[(1, 0)]
    assert list(zip(got["e_src"], got["e_dst"], got["e_w"])) == [(0, 1, _bits(2.0)), (0, 4, _bits(1.5)), (2, 3, _bits(0.0))]


# ---- 3. blocks and the worker threads ----
def _big_case():
    rng = np.random.default_rng(7)
    p = 600
    entries, off, idx, stat = [], [0], [], []
    for T in range(p):
        nb = rng.choice(p - 1, size=int(rng.integers(20, 60)), replace=False)
        nb = [int(x) + (int(x) >= T) for x in nb]
        for u in nb:
            s = math.nan if rng.random() < 0.1 else float(rng.standard_normal())
            entries.append((T, u, s, float(rng.random())))
        for u in sorted(nb):
            if rng.random() < 0.95:
                idx.append(u)
                stat.append(float(rng.standard_normal()))
        off.append(len(idx))
    assert len(entries) >= 20000
    return p, (off, idx, stat), entries


def _check_blocks(exe, env=None):
    p, l0, entries = _big_case()
    for discrete in (False, True):
        runs = _graph_runs(_run(exe, _graph_input(p, discrete, l0, entries, [(1, 1), (2, 3), (3, 2), (8, 3)]), env))
        assert sorted(runs) == [(1, 0), (2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (8, 0), (8, 1), (8, 2)]
        first = runs[(1, 0)]
        assert len(first["e_src"]) > 5000
        for key, r in runs.items():
            assert r["raw"] == first["raw"], key  # byte-identical pc_* and e_*
        if env is None:
            _same(first, _reference(p, discrete, l0, entries))
    # a block that throws: run() returns false, and only after every other block has ended; the object stays usable
    for n, k in ((8, 0), (8, 5), (2, 1), (3, 2)):
        out = _run(exe, "throw %d %d" % (n, k), env)
        assert out.split() == ["ret", "0", "ended", str(n - 1), "next", "1", "good", str(2 * n)], (n, k, out)


def test_blocks_give_identical_bytes_and_workers_are_reusable(exe):
    _check_blocks(exe)


def test_blocks_under_thread_sanitizer(tmp_path_factory, tmp_path):
    # host code only.  The flag must compile, link and start a trivial program here; otherwise the leg is skipped with the reason
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <thread>\nint main() { int x = 0; std::thread t([&] { x = 1; }); t.join(); return x - 1; }\n")
    pexe = str(tmp_path / "probe")
    c = subprocess.run(["g++", "-std=c++17", "-fsanitize=thread", "-pthread", "-o", pexe, str(probe)], capture_output=True, text=True)
    if c.returncode != 0:
        pytest.skip("g++ does not accept -fsanitize=thread here: " + c.stderr.strip()[-300:])
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=1 exitcode=66")
    r = subprocess.run([pexe], capture_output=True, text=True, env=env)
    if r.returncode != 0:
        pytest.skip("a -fsanitize=thread program does not start here: " + r.stderr.strip()[-300:])
    tsan = _compile(tmp_path_factory, "graph_check_tsan", ["-g", "-fsanitize=thread"])
    _check_blocks(tsan, env)


# ---- 4. schedule helpers ----
def _sched(exe, off, commands):
    return [[int(x) for x in ln.split()] for ln in _run(exe, "sched %d %s %s" % (len(off) - 1, " ".join(map(str, off)), " ".join(commands))).splitlines()]


def _estimate(deg, max_k):
    return float(deg) ** min(max(max_k, 1), 3) + 64.0


def test_target_order_round_ends_and_deal(exe, oracles):
    orc = oracles["fz"][0]
    nb = orc.level0(alpha=0.01, hps=5, n_obs_min=orc.auto_n_obs_min(-1, 5, 3), FDR=True)
    off = [int(x) for x in nb["off"]]
    p = len(off) - 1
    deg = np.diff(off)
    assert len(set(deg)) < p  # ties: the order has to be the stable one
    order = _sched(exe, off, ["order"])[0]
    assert order == sorted(range(p), key=lambda v: deg[v])
    # round ends: R = 1 (single_il: the first round holds two targets), 2, 16, <= 0 (one round), with max_targets cutting nt
    for R in (1, 2, 16, 0, -1):
        for nt in (p, 37, 2, 1):
            ends, r0 = [], 0
            while r0 < nt:
                r0 = _sched(exe, off, ["end %d %d %d" % (r0, R, nt)])[0][0]
                ends.append(r0)
            RR = nt if R <= 0 else R
            exp, r0 = [], 0
            while r0 < nt:
                r0 = min(nt, r0 + (2 if (RR == 1 and r0 == 0) else RR))
                exp.append(r0)
            assert ends == exp, (R, nt)
    # the deal: one owner per target, zeros for a world of one, the same on every call, and for a world of 8 never worse than round-robin
    for R in (16, 80):
        for r0 in range(0, p, R):
            r1 = min(p, r0 + R)
            assert _sched(exe, off, ["deal %d %d 1 3" % (r0, r1)])[0] == [0] * (r1 - r0)
            for world in (2, 4, 8):
                cmd = "deal %d %d %d 3" % (r0, r1, world)
                a, b = _sched(exe, off, [cmd, cmd])
                assert a == b and len(a) == r1 - r0 and all(0 <= w < world for w in a)
                est = [_estimate(deg[order[i]], 3) for i in range(r0, r1)]
                lpt = max(sum(e for e, w in zip(est, a) if w == k) for k in range(world))
                rr = max(sum(e for j, e in enumerate(est) if j % world == k) for k in range(world))
                assert lpt <= rr, (R, r0, world, lpt, rr)
                # heaviest first, each to the least loaded rank, ties to the lower rank
                load, exp = [0.0] * world, [0] * (r1 - r0)
                for j in range(r1 - r0 - 1, -1, -1):
                    exp[j] = load.index(min(load))
                    load[exp[j]] += est[j]
                assert a == exp


# ---- 5. running graph ----
def test_running_graph_whitelists_are_sorted_and_unique(exe):
    rng = np.random.default_rng(5)
    p = 30
    adds = []
    for _ in range(3):
        pairs = [(int(rng.integers(p)), int(rng.integers(p))) for _ in range(60)]
        pairs = [(t, u) for t, u in pairs if t != u]
        pairs += pairs[:10] + [(u, t) for t, u in pairs[:15]]  # duplicates and both directions
        adds.append(pairs)
    text = "running %d " % p
    exp = [set() for _ in range(p)]
    for pairs in adds:
        text += "add %d %s " % (len(pairs), " ".join("%d %d" % q for q in pairs))
        for t, u in pairs:
            exp[t].add(u)
            exp[u].add(t)
    got = [[int(x) for x in ln.split()] for ln in _run(exe, text + "lists").split("\n")[:p]]
    assert got == [sorted(s) for s in exp]
