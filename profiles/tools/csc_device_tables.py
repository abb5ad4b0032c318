"""The hand-over of a sparse table to the engine, timed: the scipy path (fw_normalize_counts_csc uploads the triple and downloads the
output triple, Engine.set_data uploads it again; the discrete kinds build their bit planes on one host thread) against the sparse-CSC
device-tensor path (fw_normalize_counts_csc_dev, fw_set_data_csc_*_dev) on the same seeded tables, alternating, in one process.  Per
configuration and path one warm-up round, then `reps` rounds of
  front-end   normalize_counts(table)                         wall seconds (the call synchronises)
  hand-over   Engine.set_data(what the front-end returned)    wall seconds, from the front-end's return to the end of set_data
  learn       learn_network(table)                            wall seconds, and from its counters t_normalize_s and the network
                                                              (t_level0_s + t_cond_s)
The networks of every round of both paths, the warm-up included, must be the same (exit status 1 otherwise).  The host-to-device copy that makes the tensor is not part
of any figure: the tensor path is for tables that are already there.
  python profiles/tools/csc_device_tables.py [out.txt] [reps] [cfg4 cfg3he ...]"""
import os
import statistics
import sys
import time

import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import flashweave_jl_amd as fw  # noqa: E402
from flashweave_jl_amd import synth  # noqa: E402
from flashweave_jl_amd.engine import is_sparse  # noqa: E402


def table(cfg):
    """-> (the configuration, its seeded count table as a canonical scipy CSC matrix)"""
    c = synth.CONFIGS[cfg]
    if c.get("habitats"):  # (the count table of the HE generator; its meta variables are not served on the device path)
        counts = synth.generate(c["p"], c["n"], c["seed"], mode=c["mode"], habitats=c["habitats"], n_meta=c["n_meta"])[0]
    else:
        counts = synth.generate(c["p"], c["n"], c["seed"], mode=c["mode"])
    m = sp.csc_matrix(counts)
    m.sort_indices()
    return c, m


def as_tensor(m):
    """the scipy CSC matrix as a sparse CSC tensor in GPU memory, over its three arrays as they are"""
    dev = torch.device("cuda", 0)
    return torch.sparse_csc_tensor(torch.from_numpy(m.indptr).to(dev), torch.from_numpy(m.indices).to(dev), torch.from_numpy(m.data).to(dev),
                                   size=m.shape)


def one_round(c, tab):
    """-> (front-end s, hand-over s, learn_network s, t_normalize_s, network s, edges)"""
    name = c["test_name"]
    t0 = time.perf_counter()
    mat = fw.normalize_counts(tab, name)[0]
    t1 = time.perf_counter()
    eng = fw.Engine(name, mat.shape[0], mat.shape[1], max_k=c["max_k"])
    t2 = time.perf_counter()
    eng.set_data((mat.indptr, mat.indices, mat.data) if is_sparse(mat) else mat)  # (the triple as it came, as learn_network hands it over)
    t3 = time.perf_counter()
    eng.close()
    del mat
    t4 = time.perf_counter()
    net = fw.learn_network(tab, sensitive=name.startswith("fz"), heterogeneous=name.endswith("_nz"), max_k=c["max_k"])
    t5 = time.perf_counter()
    cn = net["counters"]
    return t1 - t0, t3 - t2, t5 - t4, cn["t_normalize_s"], cn["t_level0_s"] + cn["t_cond_s"], net["edges"]


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else sys.stdout
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    cfgs = sys.argv[3:] or ["cfg4", "cfg3he"]

    def say(line):
        print(line, file=out, flush=True)
        if out is not sys.stdout:
            print(line, flush=True)
    say("device %s, torch %s, %d timed rounds per path after one warm-up, paths alternating" % (torch.cuda.get_device_name(0), torch.__version__, reps))
    status = 0
    for cfg in cfgs:
        c, m = table(cfg)
        tables = {"scipy": m, "tensor": as_tensor(m)}
        torch.cuda.synchronize()
        say("%s: %d samples x %d OTUs, %d stored entries (%.1f %%), %s, max_k = %d"
            % (cfg, m.shape[0], m.shape[1], m.nnz, 100.0 * m.nnz / (m.shape[0] * m.shape[1]), c["test_name"], c["max_k"]))
        rounds = {k: [] for k in tables}
        networks = []  # (of every round of both paths, the warm-up included)
        for r in range(reps + 1):
            for path, tab in tables.items():
                got = one_round(c, tab)
                networks.append(got[5])
                if r:
                    rounds[path].append(got)
                say("  %s %-6s front-end %8.4f  hand-over %8.4f  learn_network %8.4f  (t_normalize_s %8.4f, network %7.4f)  %d edges"
                    % ("warm-up" if not r else "round %d" % r, path, *got[:5], len(got[5])))
        for path in tables:
            say("  %-6s median [min .. max]: " % path + "; ".join(
                "%s %.4f [%.4f .. %.4f]" % (label, statistics.median(v), min(v), max(v))
                for label, v in zip(("front-end", "hand-over", "learn_network", "t_normalize_s", "network"), zip(*[g[:5] for g in rounds[path]]))))
        same = all(net == networks[0] for net in networks[1:])
        say("  networks of the two paths: %s" % ("the same" if same else "DIFFERENT"))  # (all 2 (reps + 1) of them)
        status |= 0 if same else 1
        del tables, m
    return status


if __name__ == "__main__":
    sys.exit(main())
