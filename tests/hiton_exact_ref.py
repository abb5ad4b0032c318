"""Python restatement of the HITON-PC driver with the reference's fast_elim / no_red_tests flags -- the checker of the exact
elimination mode (fw_learn_opts.elim_mode), which the CPU oracle's driver (oracle/fw_oracle.c, fast_elim = true only) does not have.

Built on Oracle.level0 and Oracle.test_subsets; restates si_HITON_PC (src/hiton.jl:283-400 with hiton_backend :109-149,
update_sig_result! :53-78, update_PC_dict! :249-256, the whitelist rule :20-30), the target order (learning.jl:97-98), the
feed-forward schedule (single_il: interleaved.jl:62-183, whose first round holds two targets; rounds of R targets with a whitelist
snapshot per round; feed_forward = False), make_weights and make_symmetric_graph (misc.jl:137-159, 201-272).
tests/test_exact_elim_cpu.py pins it against Oracle.learn with fast_elim = True, bit for bit.

Row views (prepare_nzdata, hiton.jl:41-50,85): the oracle's fz_nz tests take the rows of (T, candidate) themselves, and the sparse
rules of mi_nz need none (needs_nz_view, misc.jl:103-107), so each job below sees what Oracle.learn's jobs see.  Discrete
contexts must therefore be built with sparse=True."""
import math

import numpy as np

from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd import synth
from oracle import oracle as O


def _maxweight(w1, w2):
    if math.isnan(w1):
        return w2
    if math.isnan(w2):
        return w1
    s1 = (w1 > 0) - (w1 < 0)
    s2 = (w2 > 0) - (w2 < 0)
    if s1 * s2 < 0:
        return w1
    return max(abs(w1), abs(w2)) * s1


def _phase(orc, T, cands, phase, wl, support, P, fast_elim, counter):
    """hiton_backend for one phase -> OrderedDict-like {candidate: (stat, pval)} (dict keeps insertion order)."""
    acc = list(cands) if phase == "E" else []
    out = {}
    for cand in cands:
        if cand in wl:  # hiton.jl:20-30
            acc.append(cand)
            out[cand] = (math.nan, math.nan)
            continue
        if phase == "E":  # :134-136
            acc = [v for v in acc if v != cand]
        r = orc.test_subsets(T, cand, acc, max_k=P["max_k"], alpha=P["alpha"], hps=P["hps"], n_obs_min=P["n_obs_min"],
                             max_tests=P["max_tests"])
        if r["num_tests"] > 0:
            counter[0] += r["num_tests"]
        if not acc:  # :57-59
            acc.append(cand)
            out[cand] = support[cand]
        elif r["pval"] < P["alpha"] and r["suff_power"]:  # :61-63
            acc.append(cand)
            out[cand] = (r["stat"], r["pval"])
        elif phase == "E" and not fast_elim:  # :67-70
            acc.append(cand)
    return out


def si_hiton_pc(orc, T, nb, P, wl, levels, fast_elim=True, no_red_tests=True, counter=None):
    o, e = int(nb["off"][T]), int(nb["off"][T + 1])
    univar = {int(nb["idx"][i]): (float(nb["stat"][i]), float(nb["pval"][i])) for i in range(o, e)}
    if P["max_k"] == 0:
        return dict(univar)
    if levels is not None and levels[T] < 2:
        return {}
    cands = [v for v, (_, pv) in univar.items() if pv < P["alpha"]]
    cands.sort(key=lambda v: univar[v][1])  # stable
    if not cands:
        return {}
    TPC = _phase(orc, T, cands, "I", wl, univar, P, fast_elim, counter)
    PC = _phase(orc, T, list(TPC), "E", wl, TPC, P, fast_elim, counter)
    if no_red_tests or fast_elim:  # hiton.jl:388-390 -> update_PC_dict!
        for k, (s, pv) in PC.items():
            if k in TPC and (TPC[k][1] > pv or math.isnan(pv)):
                PC[k] = TPC[k]
    return PC


def learn(orc, discrete, max_k=3, alpha=0.01, hps=5, n_obs_min=-1, max_tests=10_000_000, FDR=True, feed_forward=True, round_size=1,
          fast_elim=True, no_red_tests=True):
    """LGL -> dict(pc_off, pc_idx, pc_weight, pc_pval, n_cond_tests, edges) in Oracle.learn's layout.
    round_size: 1 = single_il, R > 1 = rounds of R targets, <= 0 = one round (as fw_learn_opts.round_size)."""
    p = orc.p
    n_obs_min = orc.auto_n_obs_min(n_obs_min, hps, max_k)
    P = dict(max_k=max_k, alpha=alpha, hps=hps, n_obs_min=n_obs_min, max_tests=max_tests)
    nb = orc.level0(alpha=alpha, hps=hps, n_obs_min=n_obs_min, FDR=FDR)
    levels = orc.levels()[0] if discrete else None
    deg = np.diff(nb["off"])
    order = sorted(range(p), key=lambda v: (deg[v], v))  # learning.jl:97-98, stable
    R = p if round_size <= 0 else round_size
    adj = [[] for _ in range(p)]
    PCs = [dict() for _ in range(p)]
    counter = [0]
    r0 = 0
    while r0 < p:
        r1 = min(p, r0 + (2 if (R == 1 and r0 == 0) else R))  # single_il: the first round holds two targets
        snap = [set(a) for a in adj]
        for ti in range(r0, r1):
            T = order[ti]
            wl = snap[T] if (feed_forward and max_k > 0) else set()
            PCs[T] = si_hiton_pc(orc, T, nb, P, wl, levels, fast_elim, no_red_tests, counter)
        for ti in range(r0, r1):
            T = order[ti]
            for u in PCs[T]:
                if u not in adj[T]:
                    adj[T].append(u)
                    adj[u].append(T)
        r0 = r1
    # make_weights: discrete tests take the sign of the univariate statistic
    if discrete:
        for T in range(p):
            o, e = int(nb["off"][T]), int(nb["off"][T + 1])
            us = {int(nb["idx"][i]): float(nb["stat"][i]) for i in range(o, e)}
            for k, (s, pv) in list(PCs[T].items()):
                u = us.get(k, math.nan)
                sg = math.nan if math.isnan(u) else float((u > 0) - (u < 0))
                PCs[T][k] = (sg * abs(s), pv)
    off = np.zeros(p + 1, np.int32)
    for T in range(p):
        off[T + 1] = off[T] + len(PCs[T])
    idx = np.array([k for T in range(p) for k in PCs[T]], dtype=np.int32)
    w = np.array([v[0] for T in range(p) for v in PCs[T].values()], dtype=np.float64)
    pv = np.array([v[1] for T in range(p) for v in PCs[T].values()], dtype=np.float64)
    edges = {}
    for a in range(p):  # make_symmetric_graph, OR rule
        for b in sorted(set(PCs[a]) | {t for t in range(p) if a in PCs[t]}):
            if b <= a:
                continue
            w1 = PCs[a][b][0] if b in PCs[a] else math.nan
            w2 = PCs[b][a][0] if a in PCs[b] else math.nan
            ww = _maxweight(w1, w2)
            if not math.isnan(ww):
                edges[(a, b)] = ww
    return dict(pc_off=off, pc_idx=idx, pc_weight=w, pc_pval=pv, n_cond_tests=counter[0], n_level0_tests=nb["n_tests"], edges=edges)


def make_oracles(p=80, n=300, seed=3):
    """(kind -> (oracle, discrete, data)) on the synthetic tables the GPU tests use (fz: the Float64 Pearson matrix rounded to
    Float32 here; the GPU tests feed the device's own matrix)."""
    out = {}
    counts = synth.generate(p, n, seed, mode="S", habitats=4)
    d, _, _ = pre.normalize(counts, "fz", prec=32)
    d = np.asfortranarray(d)
    out["fz"] = (O.Oracle("fz", cor_mat=O.cor(d.astype(np.float64), "f32"), n_obs=d.shape[0]), False, d)
    d2, _, _ = pre.normalize(counts, "fz_nz", prec=32)
    d2 = np.asfortranarray(d2)
    out["fz_nz"] = (O.Oracle("fz_nz", data=d2.astype(np.float64)), False, d2)
    c3 = synth.generate(p, n, seed, mode="F")
    d3, _, _ = pre.normalize(c3, "mi")
    d3 = np.ascontiguousarray(d3)
    out["mi"] = (O.Oracle("mi", d3, sparse=True, max_k=5), True, d3)
    d4, _, _ = pre.normalize(c3, "mi_nz")
    d4 = np.ascontiguousarray(d4)
    out["mi_nz"] = (O.Oracle("mi_nz", d4, sparse=True, max_k=5), True, d4)
    return out
