"""Child process of tests/test_gpu_sparse.py::test_host_never_densifies: a 60 000 x 8 000 count table at 0.5 % fill is built
directly in CSC form and learnt with mi_nz at max_k = 0; prints one JSON line with the growth of the peak resident set
(ru_maxrss, KiB on Linux) from "library loaded" to "network returned".  ru_maxrss is a high-water mark: where importing the
libraries has already peaked above what the process holds afterwards (or where it is inherited from a larger parent), its growth
would hide an allocation, so a thread also samples the resident set itself (VmRSS) every 2 ms during the call, and the largest
sample is reported against VmRSS before the call.  What the first device call of a process maps whatever the table's size -- the
HIP runtime and the code objects of every library loaded -- is taken out of that figure by learning a small table of the same
kind first (2 000 x 300, the same code path); it is reported on its own as warmup_growth_bytes."""
import json
import os
import resource
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import scipy.sparse as sp  # noqa: E402

import flashweave_jl_amd as fw  # noqa: E402


def build_table(n=60_000, p=8_000, fill=0.005, seed=11):
    """Column by column: sorted distinct rows, log-normal counts >= 1; nothing of size n x p exists at any time."""
    rng = np.random.default_rng(seed)
    per = rng.binomial(n, fill, p)
    colptr = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in per]).astype(np.int32)
    vals = (1 + np.floor(np.exp(rng.normal(1.0, 1.5, rows.size)))).astype(np.int32)
    return sp.csc_matrix((vals, rows, colptr), shape=(n, p))


def vm_rss_kib():
    with open("/proc/self/status") as f:
        for line in f:
            if line.startswith("VmRSS:"):
                return int(line.split()[1])
    raise RuntimeError("no VmRSS in /proc/self/status")


def main():
    X = build_table()
    fw.load_library()
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    cold = vm_rss_kib()
    fw.learn_network(build_table(2_000, 300, 0.05, 12), sensitive=False, heterogeneous=True, max_k=0)
    cur0 = vm_rss_kib()
    samples, stop = [cur0], threading.Event()

    def sample():  # (ctypes releases the GIL around every library call)
        while not stop.is_set():
            samples.append(vm_rss_kib())
            time.sleep(0.002)

    th = threading.Thread(target=sample, daemon=True)
    th.start()
    net = fw.learn_network(X, sensitive=False, heterogeneous=True, max_k=0)
    stop.set()
    th.join()
    rss1 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    print(json.dumps(dict(n=X.shape[0], p=X.shape[1], nnz=int(X.nnz), rss_before_kib=rss0, rss_after_kib=rss1,
                          growth_bytes=(rss1 - rss0) * 1024, vmrss_before_kib=cur0, vmrss_peak_sampled_kib=max(samples),
                          sampled_growth_bytes=(max(samples) - cur0) * 1024, warmup_growth_bytes=(cur0 - cold) * 1024, n_samples=len(samples), dense_int32_bytes=X.shape[0] * X.shape[1] * 4,
                          edges=len(net["edges"]), variables=len(net["variable_ids"]),
                          sparse_input=bool(net["counters"]["sparse_input"]),
                          normalized_on_device=bool(net["counters"]["normalized_on_device"]))))


if __name__ == "__main__":
    main()
