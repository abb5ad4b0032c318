"""One rank of the learn_network(distributed=True) tests, and their launcher (tests/test_gpu_learn_dist.py, tests/test_learn_dist_cpu.py):
every rank on GPU 0, gloo transport.  One start runs all the cases of its world size and writes them to <out>.<rank> as JSON; floats
travel as float.hex strings, so that "to the bit" can be asked of them (NaN included)."""
import datetime
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"fz": dict(sensitive=True, heterogeneous=False), "fz_nz": dict(sensitive=True, heterogeneous=True),
         "mi": dict(sensitive=False, heterogeneous=False), "mi_nz": dict(sensitive=False, heterogeneous=True)}
ROUND_SIZES = (32, 150)


def launch(mode, world, out, limit_s=120.0):
    """Starts `world` ranks as fresh child processes and waits for all of them, at most limit_s: a rank that fails or runs out of
    time ends the others (no rank is left inside a collective), nothing is retried.  -> exit codes"""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29753 + world))
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), mode, str(r), str(world), out], env=env)
             for r in range(world)]
    deadline = time.monotonic() + limit_s
    try:
        while any(p.poll() is None for p in procs):
            if time.monotonic() > deadline or any(p.poll() not in (None, 0) for p in procs):
                break
            try:
                next(p for p in procs if p.poll() is None).wait(timeout=0.2)
            except subprocess.TimeoutExpired:
                pass
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        codes = [p.wait() for p in procs]
    return codes


def table(kind):
    """The table of tests/dist_worker.py: 300 variables x 250 samples."""
    from flashweave_jl_amd import synth
    return synth.generate(300, 250, 17, mode="S" if kind.startswith("fz") else "F")


def pack(res):
    """FWResult -> plain JSON data, floats as hex strings."""
    rej = [[int(T), int(c), [int(z) for z in zs], float(t[0]).hex(), float(t[1]).hex(), int(t[2]), bool(t[3]), int(q[0]), float(q[1]).hex()]
           for T, d in sorted(res["rejections"].items()) for c, (zs, t, q) in sorted(d.items())]
    cn = res["counters"]
    return dict(edges=sorted([int(a), int(b), float(w).hex()] for (a, b), w in res["edges"].items()), variable_ids=list(res["variable_ids"]),
                meta_variable_mask=[bool(v) for v in res["meta_variable_mask"]], rejections=rej,
                distributed=res["parameters"]["distributed"], world_size=cn["world_size"], rank=cn["rank"],
                packed_host=cn["rejections_packed_host"], packed_dev=cn["rejections_packed_dev"], received=cn["rejections_received"])


def records(rec):
    return [[int(r["target"]), int(r["candidate"]), int(r["n_zs"]), [int(z) for z in r["zs"]], int(r["df"]), int(r["suff_power"]), int(r["phase"]),
             int(r["n_acc"]), int(r["num_tests"]), float(r["frac"]).hex(), float(r["stat"]).hex(), float(r["pval"]).hex()] for r in rec]


def both(res, key, rank, data, **kw):
    """The distributed call on every rank; rank 0 then computes the one-rank baseline in the same process."""
    import flashweave_jl_amd as fw
    res[key] = pack(fw.learn_network(data, distributed=True, device=0, **kw))
    if rank == 0:
        res[key + "/single"] = pack(fw.learn_network(data, distributed=False, device=0, **kw))


def run_gpu(rank, world, out_path):
    import scipy.sparse as sp
    import torch
    import torch.distributed as dist
    import flashweave_jl_amd as fw
    from flashweave_jl_amd import preprocess as pre
    from flashweave_jl_amd.dist import make_dev_exchange
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    res = {}
    # 1. all four modes, rounds of 32 (16 or 8 targets per rank: the host job pool) and of 150 (fz kinds at world 2: device rounds)
    for kind, mode in MODES.items():
        for R in ROUND_SIZES:
            both(res, "%s/R%d" % (kind, R), rank, table(kind), max_k=3, track_rejections=True, round_size=R, **mode)
    if world == 4:
        # 2. ragged and empty contributions to the log gather
        both(res, "empty", rank, table("fz"), max_k=0, track_rejections=True, round_size=32, **MODES["fz"])
        for kind in ("fz", "mi"):  # six variables for four ranks: most ranks own no rejected candidate
            both(res, "ragged/" + kind, rank, table(kind)[:, :6], max_k=1, track_rejections=True, round_size=32, **MODES[kind])
    if world == 2:
        # 3. the CSC-resident layout of a sparse fz_nz table, sharded
        both(res, "cscres", rank, sp.csc_matrix(table("fz_nz")), max_k=3, track_rejections=True, round_size=32, csc_resident=True, **MODES["fz_nz"])
        # 6. Engine level: without gather_rejections nothing changes, with it every rank holds the union
        data, _, _ = pre.normalize(table("fz"), "fz")
        n, p = data.shape
        eng = fw.Engine("fz", n, p, max_k=3)
        eng.set_data(data)
        eng.compute_cor()
        xchg = make_dev_exchange(dist, torch.device("cuda", 0))
        try:
            eng.gather_rejections(xchg)  # (refused before any collective)
            res["engine/early"] = None
        except fw.FlashWeaveError as e:
            res["engine/early"] = e.code
        eng.level0()
        eng.lgl(feed_forward=True, round_size=32, rank=rank, world_size=world, dev_exchange=xchg, track_rejections=True)
        res["engine/own"] = records(eng.rejection_records())
        res["engine/stats"] = eng.gather_rejections(xchg)
        res["engine/all"] = records(eng.rejection_records())
        res["engine/again"] = eng.gather_rejections(xchg)  # a no-op: no collective, the same log
        res["engine/all2"] = records(eng.rejection_records())
        eng.close()
        if rank == 0:
            one = fw.Engine("fz", n, p, max_k=3)
            one.set_data(data)
            one.compute_cor()
            one.lgl(feed_forward=True, round_size=32, track_rejections=True)
            res["engine/single"] = records(one.rejection_records())
            one.close()
        # 4. the input check: rank 1 holds the table with one count changed
        counts = table("mi")
        if rank == 1:
            counts = counts.copy()
            counts[3, 5] += 1
        try:
            fw.learn_network(counts, distributed=True, device=0, max_k=3, **MODES["mi"])
            res["mismatch"] = None
        except ValueError as e:
            res["mismatch"] = str(e)
    json.dump(res, open(out_path + ".%d" % rank, "w"))
    dist.barrier()
    dist.destroy_process_group()


def run_cpu_refusal(rank, world, out_path):
    """prec=64 with the plain fz test inside a gloo group of CPU processes: refused by name before any engine exists."""
    import torch.distributed as dist
    import flashweave_jl_amd as fw
    from flashweave_jl_amd import api
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    made = []

    class NoEngine:
        def __init__(self, *a, **k):
            made.append(1)
            raise AssertionError("an engine was created")
    api.Engine = NoEngine
    msg = None
    try:
        fw.learn_network(np.ones((8, 4), np.int32), distributed=True, prec=64, sensitive=True, heterogeneous=False)
    except ValueError as e:
        msg = str(e)
    json.dump(dict(message=msg, engines=len(made)), open(out_path + ".%d" % rank, "w"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    mode, rank, world, out = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    (run_gpu if mode == "gpu" else run_cpu_refusal)(rank, world, out)
