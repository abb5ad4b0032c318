"""Child process of tests/test_gpu_cscres.py::test_device_never_holds_the_dense_matrix: a 40 000 x 3 000 Float32 table at 1 % fill
(4 n p = 480 MB dense) is built directly in CSC form, uploaded CSC-resident and learnt with fz_nz; prints one JSON line with the
largest drop of the device's free memory (torch.cuda.mem_get_info) between "before the upload" and the points after the upload,
after level 0 and after the network, with the engine still open.  What the first device calls of a process allocate whatever the
table's size (runtime, code objects, staging streams) is taken out by learning a small table in both layouts first.  The same
figure for a dense-resident upload of the same table follows, to show that the measurement sees a matrix of that size."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import flashweave_jl_amd as fw  # noqa: E402


def build_triple(n, p, fill, seed):
    """Column by column: sorted distinct rows, values around 2 (never 0); nothing of size n x p exists at any time."""
    rng = np.random.default_rng(seed)
    per = rng.binomial(n, fill, p)
    colptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in per]).astype(np.int32)
    vals = (2.0 + rng.standard_normal(rows.size)).astype(np.float32)
    vals[vals == 0.0] = 1.0
    return colptr, rows, vals


def free_bytes():
    torch.cuda.synchronize()
    return int(torch.cuda.mem_get_info()[0])


def run(n, p, triple, csc_resident, measure):
    eng = fw.Engine("fz_nz", n, p, max_k=3)
    try:
        before = free_bytes() if measure else 0
        if csc_resident:
            eng.set_data(triple, csc_resident=True)
        else:
            eng.set_data(triple)
        low = free_bytes() if measure else 0
        resident = eng.data_resident_bytes()
        eng.level0()
        low = min(low, free_bytes()) if measure else 0
        net = eng.lgl(feed_forward=True, round_size=0, edge_dict=False)
        low = min(low, free_bytes()) if measure else 0
        return dict(drop=before - low, resident=resident, edges=int(len(net["edge_src"])))
    finally:
        eng.close()


def main():
    n, p = 40_000, 3_000
    small = build_triple(2_000, 300, 0.03, 5)
    for layout in (True, False):
        run(2_000, 300, small, layout, False)
    triple = build_triple(n, p, 0.01, 6)
    csc = run(n, p, triple, True, True)
    dense = run(n, p, triple, False, True)
    print(json.dumps(dict(n=n, p=p, nnz=int(triple[0][-1]), dense_matrix_bytes=4 * n * p, csc_drop_bytes=csc["drop"],
                          csc_resident_bytes=csc["resident"], dense_drop_bytes=dense["drop"], dense_resident_bytes=dense["resident"],
                          csc_edges=csc["edges"], dense_edges=dense["edges"])))


if __name__ == "__main__":
    main()
