"""Discrete runs under knobs the library reads once per process (FW_MI_ROWK, FW_MI_ROW4: `static const` in the library), started as a
child process by tests/test_gpu_mi_edges.py -- one child at a time, the knobs in its environment.  The tables are that module's
generators, so parent and child hold the same bytes.  Prints one JSON line.

usage: FW_DEV_MIN_TARGETS=1 FW_MI_ROW4=2 python tests/mi_edges_worker.py --mode net --kinds mi,mi_nz --ns 2049,5120 --max-k 3
           {"<kind>:<n>": {edges, edge_weight, pc_off, pc_idx, pc_weight, cond_tests_ref, level0_tests}}   (`chain`, feed_forward = False)
       FW_MI_ROWK=99 python tests/mi_edges_worker.py --mode single --kinds mi_nz --ns 505,511
           {"<kind>:<n>:<dense rules 0 | 1>": [[stat, pval, df, suff_power], ...]}                         (`dependent`, the 240 jobs)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("FW_KNOBS", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("net", "single"), required=True)
    ap.add_argument("--kinds", default="mi,mi_nz")
    ap.add_argument("--ns", required=True)
    ap.add_argument("--max-k", type=int, default=3)
    a = ap.parse_args()
    from tests import test_gpu_mi_edges as E
    out = {}
    for kind in a.kinds.split(","):
        for n in (int(v) for v in a.ns.split(",")):
            if a.mode == "net":
                out["%s:%d" % (kind, n)] = E.network_result(kind, n, a.max_k)
            else:
                for dense in (0, 1):
                    out["%s:%d:%d" % (kind, n, dense)] = E.single_result(kind, n, bool(dense))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
