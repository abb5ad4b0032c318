"""csrc/fw_level0_host.h -- the host-only part of level 0 (Benjamini-Hochberg on the significant pairs, neighbour CSR, split of an
all-gathered record list; what FW_HOST_BH=1 and fw_level0_sharded run) -- compiled natively through tests/native/level0_check.cpp: no GPU,
no build of the library.

Doubles cross the text boundary as the hex digits of their bits and are compared as bits.  BH is compared with
oracle.benjamini_hochberg, whose expression `p * m / (i + 1)` and clamp of the last element are the header's own; the oracle only
adjusts p < alpha, so it is called with alpha = 2.  The gather split returns the number of count records it met; turning a count other
than `world` into FW_ERR_ARG ("%d of %d ranks reported") is l0_exchange_host's step in fw_core.cpp, which needs a context and so a GPU
(tests/test_gpu_dist.py and tests/test_gpu_learn_dist.py run the exchange itself)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "level0_check.cpp")
HEADER = os.path.join(ROOT, "flashweave.jl_amd", "csrc", "fw_level0_host.h")


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _hex(x):
    return "%016x" % _bits(x)


def _hexes(v):
    return ["%016x" % b for b in np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("level0_check") / "level0_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-o", out, SRC], check=True)
    return out


def _run(exe, tokens):
    r = subprocess.run([exe], input=" ".join(map(str, tokens)), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    return r.stdout.split("\n")


def test_header_compiles_without_hip(tmp_path):
    # plain g++, nothing on the include path: the header and everything it includes is host C++, and none of it is a HIP header
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "%s"\nint main() { return 0; }\n' % HEADER)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-H", str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    included = [ln for ln in r.stderr.splitlines() if ln.startswith(".")]  # -H: one line per header, dots for the depth
    assert included and not [ln for ln in included if "hip" in ln.lower()]


# ---- 1. Benjamini-Hochberg ----
def _bh(exe, p, m):
    out = _run(exe, ["bh", len(p), m, *_hexes(p)])
    return [int(x, 16) for x in out[0].split()]


def _bh_cases():
    rng = np.random.default_rng(11)
    sub = 5e-324 * 12345  # a subnormal
    ties = np.repeat(rng.random(7) * 1e-3, [1, 4, 2, 9, 1, 3, 5])
    rng.shuffle(ties)
    return {
        "empty": (np.zeros(0), 10), "one": (np.array([0.003]), 1), "one_big_m": (np.array([0.003]), 10**7),
        "all_equal": (np.full(40, 1e-5), 40), "tie_runs": (ties, 1000), "zero_one_subnormal": (np.array([0.0, 1.0, sub, 0.5, 0.0, sub, 1.0]), 7),
        "m_eq_k": (rng.random(500), 500), "m_much_larger": (rng.random(500) * 1e-9, 12_497_500), "above_one": (np.array([0.9, 0.95, 0.99]), 100),
    }


@pytest.mark.parametrize("name", sorted(_bh_cases()))
def test_bh_equals_the_oracle_to_the_bit(exe, name):
    p, m = _bh_cases()[name]
    got = _bh(exe, p, m)
    exp = O.benjamini_hochberg(p, alpha=2.0, m=m)
    assert got == [int(b) for b in exp.view(np.uint64)]
    if len(p):
        assert max(exp) <= 1.0


def test_bh_70000_values_over_many_exponents(exe):
    # 10 ** uniform(-300, 0): the keys differ in all four 16-bit digits, so every radix pass moves data
    rng = np.random.default_rng(12)
    k = 70_000
    p = 10.0 ** rng.uniform(-300.0, 0.0, k)
    p[rng.integers(0, k, 2000)] = p[rng.integers(0, k, 2000)]  # and ties
    keys = p.view(np.uint64)
    for sh in (0, 16, 32, 48):
        assert len(np.unique((keys >> np.uint64(sh)) & np.uint64(0xFFFF))) > 300, sh
    got = _bh(exe, p, 3 * k)
    exp = O.benjamini_hochberg(p, alpha=2.0, m=3 * k)
    assert got == [int(b) for b in exp.view(np.uint64)]


# ---- 2. neighbour lists ----
def _csr(exe, p, pi, pj, stat, adj, alpha=0.01):
    out = _run(exe, ["csr", p, len(pi), _hex(alpha), *pi, *pj, *_hexes(stat), *_hexes(adj)])
    return ([int(x) for x in out[0].split()], [int(x) for x in out[1].split()], [int(x, 16) for x in out[2].split()],
            [int(x, 16) for x in out[3].split()])


def _csr_ref(p, pi, pj, stat, adj, alpha=0.01):
    """both directions of every pair with adjusted p < alpha, ascending (variable, partner)"""
    ent = []
    for i, j, s, q in zip(pi, pj, stat, adj):
        if q < alpha:
            ent += [(i, j, s, q), (j, i, s, q)]
    ent.sort(key=lambda e: (e[0], e[1]))
    off = np.zeros(p + 1, dtype=np.int64)
    for e in ent:
        off[e[0] + 1] += 1
    return ([int(x) for x in np.cumsum(off)], [e[1] for e in ent], [_bits(e[2]) for e in ent], [_bits(e[3]) for e in ent])


def _pairs(rng, p, frac_sig):
    pi, pj = np.triu_indices(p, 1)
    stat = rng.standard_normal(len(pi))
    adj = np.where(rng.random(len(pi)) < frac_sig, rng.random(len(pi)) * 0.0099, 0.01 + rng.random(len(pi)))
    return [int(x) for x in pi], [int(x) for x in pj], stat, adj


@pytest.mark.parametrize("p,frac", [(1, 0.5), (2, 1.0), (5, 0.5), (5, 0.0), (5, 1.0), (37, 0.3)])
def test_csr_equals_numpy_in_any_pair_order(exe, p, frac):
    rng = np.random.default_rng(100 + p)
    pi, pj, stat, adj = _pairs(rng, p, frac)
    if p == 5 and frac == 0.5:  # variable 3 isolated; alpha itself is not below alpha
        adj = np.where((np.array(pi) == 3) | (np.array(pj) == 3), 0.5, adj)
        adj[0] = 0.01
    ref = _csr_ref(p, pi, pj, stat, adj)
    if p == 5 and frac == 0.5:
        assert ref[0][3] == ref[0][4] and 0 < ref[0][5] < 20
    if frac == 0.0:
        assert ref[0] == [0] * (p + 1)
    if frac == 1.0:
        assert ref[0][-1] == p * (p - 1)
    assert _csr(exe, p, pi, pj, stat, adj) == ref
    for seed in (1, 2):  # a sharded merge delivers the pairs in any order: identical lists
        o = np.random.default_rng(seed).permutation(len(pi))
        assert _csr(exe, p, [pi[t] for t in o], [pj[t] for t in o], stat[o], adj[o]) == ref


# ---- 3. split of an all-gathered list ----
def _split(exe, world, npairs, recs):
    tok = ["split", world, npairs, len(recs)]
    for i, j, s, q in recs:
        tok += [i, j, _hex(s), _hex(q)]
    out = _run(exe, tok)
    nrec, m, k = (int(x) for x in out[0].split())
    return nrec, m, ([int(x) for x in out[1].split()], [int(x) for x in out[2].split()], [int(x, 16) for x in out[3].split()],
                     [int(x, 16) for x in out[4].split()])


@pytest.mark.parametrize("world", [1, 2, 3])
def test_gather_split_and_the_m_rule(exe, world):
    rng = np.random.default_rng(world)
    p = 12
    npairs = p * (p - 1) // 2
    unreliable = [int(rng.integers(0, 5)) for _ in range(world)]
    recs, pairs = [], []
    for r in range(world):  # each rank: its pairs, then its count record (npairs minus ITS unreliable pairs)
        mine = [(int(i), int(j), float(rng.standard_normal()), float(rng.random())) for i in range(p) for j in range(i + 1, p) if (i + j) % world == r and rng.random() < 0.4]
        recs += mine + [(-1, r, float(npairs - unreliable[r]), 0.0)]
        pairs += mine
    nrec, m, got = _split(exe, world, npairs, recs)
    assert nrec == world
    assert m == sum(npairs - u for u in unreliable) - (world - 1) * npairs == npairs - sum(unreliable)
    assert got == ([e[0] for e in pairs], [e[1] for e in pairs], [_bits(e[2]) for e in pairs], [_bits(e[3]) for e in pairs])
    # a missing and a doubled count record: the count the caller turns into an error
    count_at = [t for t, e in enumerate(recs) if e[0] < 0]
    assert _split(exe, world, npairs, recs[:count_at[0]] + recs[count_at[0] + 1:])[0] == world - 1
    assert _split(exe, world, npairs, recs + [recs[count_at[-1]]])[0] == world + 1


def test_gather_split_of_nothing(exe):
    assert _split(exe, 1, 6, []) == (0, 0, ([], [], [], []))
    assert _split(exe, 1, 6, [(-1, 0, 6.0, 0.0)]) == (1, 6, ([], [], [], []))
