"""Ten neighbourhoods against the whole network, in a mode that takes the host job pool (fz, prec=64): medians of three, after a warm-up
of each call, alternating the two; written as it goes.
    python profiles/tools/neighbors_timing.py P N [OUT]     (OUT defaults to profiles/neighbors.txt)"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.getcwd())
import flashweave_jl_amd as fw
from flashweave_jl_amd import preprocess as pre, synth

P, N, SEED = int(sys.argv[1]), int(sys.argv[2]), 3
out = open(sys.argv[3] if len(sys.argv) > 3 else "profiles/neighbors.txt", "w")
def say(s):
    print(s); out.write(s + "\n"); out.flush()
data, _, _ = pre.normalize(synth.generate(P, N, SEED, mode="S"), "fz", prec=64)
n, p = data.shape
eng = fw.Engine("fz", n, p, max_k=3, prec=64)
eng.set_data(np.asarray(data, dtype=np.float64)); eng.compute_cor(); eng.level0()
deg = np.diff(eng.pw_univar_neighbors()["off"])
order = np.argsort(deg, kind="stable")
targets = [int(v) for v in order[np.linspace(0, p - 1, 10).astype(int)]]  # ten targets spread over the schedule, lightest to heaviest
say("fz prec=64 (host job pool), synth.generate(%d, %d, %d, mode='S') -> n=%d p=%d, level-0 degrees min/median/max %d/%d/%d; targets' degrees %s"
    % (P, N, SEED, n, p, deg.min(), int(np.median(deg)), deg.max(), [int(deg[t]) for t in targets]))
def timed(f):
    t0 = time.perf_counter(); r = f(); return time.perf_counter() - t0, r
w_nb, nb = timed(lambda: eng.neighbors(targets, edge_dict=False))
say("warm-up neighbors(10): %.4f s" % w_nb)
w_full, full = timed(lambda: eng.lgl(feed_forward=False, round_size=0, edge_dict=False))
say("warm-up lgl(feed_forward=False): %.4f s" % w_full)
for t in targets:  # same rows
    a, b = nb["pc_off"], full["pc_off"]
    assert all(nb[k][a[t]:a[t + 1]].tobytes() == full[k][b[t]:b[t + 1]].tobytes() for k in ("pc_idx", "pc_weight", "pc_pval")), t
t_nb, t_full = [], []
for i in range(3):
    eng.reset_counters()
    t_nb.append(timed(lambda: eng.neighbors(targets, edge_dict=False))[0]); c_nb = eng.counters()
    eng.reset_counters()
    t_full.append(timed(lambda: eng.lgl(feed_forward=False, round_size=0, edge_dict=False))[0]); c_full = eng.counters()
    say("run %d: neighbors(10) %.4f s, whole network %.4f s" % (i + 1, t_nb[-1], t_full[-1]))
say("medians of three: neighbors(10) %.4f s (%d conditional tests in reference order), whole network %.4f s (%d tests): %.1f x"
    % (np.median(t_nb), c_nb["cond_tests_ref"], np.median(t_full), c_full["cond_tests_ref"], np.median(t_full) / np.median(t_nb)))
eng.close()
