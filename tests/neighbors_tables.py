"""Tables and target lists of the learn_neighbors tests: a helper module, not a test (tests/test_neighbors_cpu.py checks on the oracle
that the tables hold what the comparisons need, tests/test_gpu_neighbors.py runs them).

A table is synth.generate's, normalised on the host, plus four crafted columns at its end, so that every kind has what the synthetic
communities alone do not give at these sizes -- variables without a level-0 neighbour and with exactly one:
    p - 4, p - 3    independent noise: no neighbour
    p - 2, p - 1    noise and a noisy copy of it: each the other's only neighbour
fz_nz keeps synth's columns alone (its level-0 lists are short enough to hold all of that already)."""
import numpy as np

from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd import synth

KINDS = ("fz", "fz_nz", "mi", "mi_nz")
SIZES = {40: 200, 130: 260}  # p -> n: the sizes of the existing edge tests
N_MI_NZ = 400                # mi_nz reads the rows where both variables are present and needs n_obs_min = 160 of them: no power below


def table(kind, p, seed=5):
    """-> the n x p matrix an Engine of `kind` takes (rows may be fewer than SIZES[p]: normalisation drops empty samples)"""
    n = N_MI_NZ if kind == "mi_nz" else SIZES[p]
    if kind == "fz_nz":
        data, _, _ = pre.normalize(synth.generate(p, n, seed, mode="S", habitats=4), "fz_nz", prec=32)
        return np.asfortranarray(data)
    rng = np.random.default_rng([seed, p])
    counts = synth.generate(p - 4, n, seed, mode="S" if kind == "fz" else "F")
    data, _, _ = pre.normalize(counts, kind, prec=32) if kind == "fz" else pre.normalize(counts, kind)
    rows = data.shape[0]
    if kind == "fz":
        z = rng.standard_normal((rows, 3))
        extra = np.stack([z[:, 0], z[:, 1], z[:, 2], z[:, 2] + 0.3 * rng.standard_normal(rows)], axis=1)
        return np.asfortranarray(np.concatenate([data, extra.astype(np.float32)], axis=1))
    # discrete: levels 1 / 2 for mi_nz (a zero is an absence there, and the test reads the rows where both are present), 0 / 1 for mi
    lo = 1 if kind == "mi_nz" else 0
    b = rng.integers(0, 2, size=(rows, 3))
    copy = np.where(rng.random(rows) < 0.08, 1 - b[:, 2], b[:, 2])
    extra = np.stack([b[:, 0], b[:, 1], b[:, 2], copy], axis=1) + lo
    return np.ascontiguousarray(np.concatenate([data, extra.astype(data.dtype)], axis=1))


def choose_targets(off, idx):
    """The target lists of the issue from level-0 neighbour lists (CSR) -> dict of lists:
    longest: the variable with the longest list; single: one with a single neighbour; none: one without any; pair: two level-0
    neighbours (the heaviest variable and its first neighbour); all: every variable.  A KeyError-free dict: a missing kind of variable
    gives an empty list, which the tests refuse."""
    deg = np.diff(np.asarray(off))
    p = deg.size
    top = int(np.argmax(deg))
    single = [int(v) for v in np.nonzero(deg == 1)[0][:1]]
    none = [int(v) for v in np.nonzero(deg == 0)[0][:1]]
    pair = [top, int(idx[off[top]])] if deg[top] > 0 else []
    return dict(longest=[top], single=single, none=none, pair=pair, all=list(range(p)))


def symmetric_graph(pc_off, pc_idx, pc_weight):
    """make_symmetric_graph (misc.jl:201-272) of directed rows, written out plainly: {(a, b): weight} with a < b under the OR rule,
    the two directions merged by maxweight (a NaN gives way, opposite signs keep the lower endpoint's direction, else the larger
    magnitude), NaN edges dropped."""
    d = {}
    for t in range(len(pc_off) - 1):
        for q in range(int(pc_off[t]), int(pc_off[t + 1])):
            d[(t, int(pc_idx[q]))] = float(pc_weight[q])

    def maxweight(w1, w2):
        if np.isnan(w1):
            return w2
        if np.isnan(w2):
            return w1
        if np.sign(w1) * np.sign(w2) < 0:
            return w1
        return max(abs(w1), abs(w2)) * np.sign(w1)
    edges = {}
    for (a, b), w in d.items():
        lo, hi = min(a, b), max(a, b)
        if (lo, hi) in edges:
            continue
        ww = maxweight(d.get((lo, hi), np.nan), d.get((hi, lo), np.nan))
        if not np.isnan(ww):
            edges[(lo, hi)] = float(ww)
    return edges


def rows_of(net, targets):
    """the directed rows of `targets` in a result of Engine.lgl / Engine.neighbors -> {t: (idx bytes, weight bytes, pval bytes)}"""
    off = net["pc_off"]
    return {int(t): tuple(net[k][off[t]:off[t + 1]].tobytes() for k in ("pc_idx", "pc_weight", "pc_pval")) for t in targets}
