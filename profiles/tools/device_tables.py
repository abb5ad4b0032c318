"""The hand-over of a dense table to the engine, timed: the numpy path (front-end downloads, set_data repacks on the host and uploads)
against the device-tensor path (fw_normalize_counts_dev, fw_set_data_dense_*_dev) on the same seeded tables, alternating, in one
process.  Per configuration and path one warm-up round, then `reps` rounds of
  front-end   normalize_counts(table)                         wall seconds (the call synchronises)
  hand-over   Engine.set_data(what the front-end returned)    wall seconds, from the front-end's return to the end of set_data
  learn       learn_network(table)                            wall seconds, and from its counters t_normalize_s and the network
                                                              (t_level0_s + t_cond_s)
The networks of the two paths must be the same (exit status 1 otherwise).  The host-to-device copy that makes the tensor is not part
of any figure: the tensor path is for tables that are already there.
  python profiles/tools/device_tables.py [out.txt] [reps] [cfg4 cfg3 ...]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import flashweave_jl_amd as fw  # noqa: E402
from flashweave_jl_amd import synth  # noqa: E402


def table(cfg):
    c = synth.CONFIGS[cfg]
    if c.get("habitats"):  # (the count table of the HE generator; its meta variables are not served on the device path)
        return c, synth.generate(c["p"], c["n"], c["seed"], mode=c["mode"], habitats=c["habitats"], n_meta=c["n_meta"])[0]
    return c, synth.generate(c["p"], c["n"], c["seed"], mode=c["mode"])


def one_round(c, tab):
    """-> (front-end s, hand-over s, learn_network s, t_normalize_s, network s, edges)"""
    name = c["test_name"]
    t0 = time.perf_counter()
    mat = fw.normalize_counts(tab, name)[0]
    t1 = time.perf_counter()
    eng = fw.Engine(name, mat.shape[0], mat.shape[1], max_k=c["max_k"])
    t2 = time.perf_counter()
    eng.set_data(mat)
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
    cfgs = sys.argv[3:] or ["cfg4", "cfg3"]

    def say(line):
        print(line, file=out, flush=True)
        if out is not sys.stdout:
            print(line, flush=True)
    say("device %s, torch %s, %d timed rounds per path after one warm-up, paths alternating" % (torch.cuda.get_device_name(0), torch.__version__, reps))
    status = 0
    for cfg in cfgs:
        c, counts = table(cfg)
        tables = {"numpy": counts, "tensor": torch.from_numpy(counts).to("cuda:0")}
        torch.cuda.synchronize()
        say("%s: %d samples x %d OTUs, %s, max_k = %d" % (cfg, counts.shape[0], counts.shape[1], c["test_name"], c["max_k"]))
        rounds = {k: [] for k in tables}
        for r in range(reps + 1):
            for path, tab in tables.items():
                got = one_round(c, tab)
                if r:
                    rounds[path].append(got)
                say("  %s %-6s front-end %8.4f  hand-over %8.4f  learn_network %8.4f  (t_normalize_s %8.4f, network %7.4f)  %d edges"
                    % ("warm-up" if not r else "round %d" % r, path, *got[:5], len(got[5])))
        for path in tables:
            say("  %-6s median [min .. max]: " % path + "; ".join(
                "%s %.4f [%.4f .. %.4f]" % (label, statistics.median(v), min(v), max(v))
                for label, v in zip(("front-end", "hand-over", "learn_network", "t_normalize_s", "network"), zip(*[g[:5] for g in rounds[path]]))))
        same = rounds["numpy"][0][5] == rounds["tensor"][0][5]
        say("  networks of the two paths: %s" % ("the same" if same else "DIFFERENT"))
        status |= 0 if same else 1
        del tables, counts
    return status


if __name__ == "__main__":
    sys.exit(main())
