"""fz_nz: the dense-resident and the CSC-resident layout against each other on one workload -- synth's HE table (habitat-wise
structural absences) at p = 3000 OTUs, n = 2000 samples, max_k = 3, the default schedule of device rounds.  For each layout: upload,
one warm-up network, then `reps` networks from a fresh upload each; level-0 and conditional seconds are the library's own counters
(t_level0_s, t_cond_s), reported as median and range.  The networks of the two layouts must be the same bytes.
usage: python profiles/tools/cscres_layouts.py [out.json] [reps]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

import flashweave_jl_amd as fw  # noqa: E402
from flashweave_jl_amd import synth  # noqa: E402
from flashweave_jl_amd.api import default_round_size  # noqa: E402

NET_KEYS = ("pc_off", "pc_idx", "pc_weight", "pc_pval", "edge_src", "edge_dst", "edge_weight")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    counts = synth.generate(3000, 2000, 20260934, mode="S", habitats=4)
    mat, _, _ = fw.normalize_counts(sp.csc_matrix(counts), "fz_nz")
    n, p = mat.shape
    triple = (mat.indptr.astype(np.int64), mat.indices.astype(np.int32), mat.data.astype(np.float32))
    R = default_round_size(p)
    res = dict(n=n, p=p, nnz=int(np.count_nonzero(mat.data)), fill=float(np.count_nonzero(mat.data)) / (n * p), round_size=R, reps=reps, layouts={})
    nets = {}
    for layout in ("dense", "csc"):
        eng = fw.Engine("fz_nz", n, p, max_k=3)
        try:
            l0, cond = [], []
            for rep in range(reps + 1):  # (rep 0: warm-up, not reported)
                eng.set_data(triple, csc_resident=(layout == "csc"))
                eng.reset_counters()
                net = eng.lgl(feed_forward=True, round_size=R, edge_dict=False)
                c = eng.counters()
                if rep:
                    l0.append(c["t_level0_s"])
                    cond.append(c["t_cond_s"])
            nets[layout] = {k: net[k].tobytes() for k in NET_KEYS}
            res["layouts"][layout] = dict(resident_bytes=eng.data_resident_bytes(), edges=int(len(net["edge_src"])),
                                          cond_tests=int(c["cond_tests_ref"]),
                                          level0_ms=dict(median=1e3 * statistics.median(l0), min=1e3 * min(l0), max=1e3 * max(l0)),
                                          cond_ms=dict(median=1e3 * statistics.median(cond), min=1e3 * min(cond), max=1e3 * max(cond)))
        finally:
            eng.close()
    res["same_network"] = nets["dense"] == nets["csc"]
    text = json.dumps(res, indent=1)
    print(text)
    if out_path:
        with open(out_path, "w") as f:
            f.write(text + "\n")
    return 0 if res["same_network"] else 1


if __name__ == "__main__":
    sys.exit(main())
