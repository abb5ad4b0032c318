"""learn_network(distributed=True) with 2 and 4 ranks (all on GPU 0, gloo transport) against the one-rank call, and the rejection-log
gather underneath it (fw_rejections_allgather_dev / _comm, csrc/fw_xchg.hip).

One start of tests/learn_dist_worker.py per world size runs every case of that world (a fresh process per rank, a few seconds of set-up
each); the tests below read what the ranks wrote.  Rank 0 computes the one-rank baseline in the same process.  Fisher-z kinds are held
to the bit; the discrete kinds to the tolerances of tests/test_gpu_dist.py (a rank with few targets runs them through the host pool,
one test per wavefront, the single rank through the persistent kernel: statistics to the summation order, 1e-12 relative; p-values
1e-10 relative, the figure the discrete p-values are held to against the oracle)."""
import json
import os
import tempfile
import time

import numpy as np
import pytest

from tests.learn_dist_worker import MODES, ROUND_SIZES, launch

pytestmark = pytest.mark.gpu

FZ = ("fz", "fz_nz")


@pytest.fixture(scope="module")
def runs():
    """world -> [what rank r wrote]; each world starts once, on first use."""
    got = {}

    def get(world):
        if world not in got:
            with tempfile.TemporaryDirectory() as d:
                out = os.path.join(d, "res")
                t0 = time.monotonic()
                codes = launch("gpu", world, out)
                print("world %d: %.1f s" % (world, time.monotonic() - t0))
                assert codes == [0] * world, codes
                got[world] = [json.load(open("%s.%d" % (out, r))) for r in range(world)]
        return got[world]
    return get


def same_everywhere(ranks, key):
    for r in ranks[1:]:
        for f in ("edges", "variable_ids", "meta_variable_mask", "rejections"):
            assert r[key][f] == ranks[0][key][f], (key, f)


def close(a, b, tol):
    a, b = float.fromhex(a), float.fromhex(b)
    return a == b or (np.isnan(a) and np.isnan(b)) or abs(a - b) <= tol * abs(b)


def against_single(ranks, key, exact):
    got, one = ranks[0][key], ranks[0][key + "/single"]
    assert got["variable_ids"] == one["variable_ids"] and got["meta_variable_mask"] == one["meta_variable_mask"]
    if exact:
        assert got["edges"] == one["edges"] and got["rejections"] == one["rejections"]
        return
    assert [e[:2] for e in got["edges"]] == [e[:2] for e in one["edges"]]
    assert all(close(a[2], b[2], 1e-12) for a, b in zip(got["edges"], one["edges"]))
    assert [r[:3] for r in got["rejections"]] == [r[:3] for r in one["rejections"]]  # keys and conditioning sets
    for a, b in zip(got["rejections"], one["rejections"]):
        assert a[5:] == b[5:], (a, b)  # df, suff_power, num_tests, frac
        assert close(a[3], b[3], 1e-12) and close(a[4], b[4], 1e-10), (a, b)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("kind", list(MODES))
@pytest.mark.parametrize("R", ROUND_SIZES)
def test_distributed_equals_single(runs, world, kind, R):
    ranks, key = runs(world), "%s/R%d" % (kind, R)
    same_everywhere(ranks, key)
    against_single(ranks, key, exact=kind in FZ)
    assert len(ranks[0][key + "/single"]["rejections"]) > 0 and len(ranks[0][key]["edges"]) > 0
    for r, res in enumerate(ranks):
        assert (res[key]["distributed"], res[key]["world_size"], res[key]["rank"]) == (world, world, r)
    assert ranks[0][key + "/single"]["distributed"] == 0 and ranks[0][key + "/single"]["packed_host"] is None
    # every rank packed its own records, and received the others'
    total = len(ranks[0][key]["rejections"])
    assert sum(res[key]["packed_host"] + res[key]["packed_dev"] for res in ranks) == total
    assert all(res[key]["packed_host"] + res[key]["packed_dev"] + res[key]["received"] == total for res in ranks)
    print(key, "world", world, [(res[key]["packed_host"], res[key]["packed_dev"]) for res in ranks])


def test_both_kinds_of_slot_were_packed(runs):
    """Rounds of 32 targets leave 16 per rank at world 2: the host job pool (fewer than FW_DEV_MIN_TARGETS = 64), whose records reach
    the device slots through the upload; of a round of 150 at least one rank holds 75 or more: device rounds, whose records are in
    the device slots already.  Both went through the pack kernel."""
    ranks = runs(2)
    for kind in FZ:
        assert sum(res[kind + "/R32"]["packed_host"] for res in ranks) > 0 and sum(res[kind + "/R32"]["packed_dev"] for res in ranks) == 0
    assert sum(res["fz/R150"]["packed_dev"] for res in ranks) > 0


@pytest.mark.parametrize("key", ["empty", "ragged/fz", "ragged/mi"])
def test_ragged_and_empty_contributions(runs, key):
    ranks = runs(4)
    same_everywhere(ranks, key)
    against_single(ranks, key, exact=not key.endswith("mi"))
    if key == "empty":
        assert all(res[key]["rejections"] == [] for res in ranks) and len(ranks[0][key]["edges"]) > 0
    print(key, [(res[key]["packed_host"], res[key]["packed_dev"]) for res in ranks])


def test_csc_resident_sharded(runs):
    """The sharded run of the CSC-resident fz_nz layout: network and log are the bytes of the one-rank CSC-resident run."""
    ranks = runs(2)
    same_everywhere(ranks, "cscres")
    against_single(ranks, "cscres", exact=True)
    assert len(ranks[0]["cscres"]["rejections"]) > 0


def test_input_check(runs):
    """Rank 1 held the table with one count changed: both ranks raise ValueError naming distributed (and both processes ended)."""
    for res in runs(2):
        assert res["mismatch"] is not None and "distributed" in res["mismatch"]


def test_engine_level_gather(runs):
    ranks = runs(2)
    single = ranks[0]["engine/single"]
    assert all(res["engine/early"] == -3 for res in ranks)  # FW_ERR_STATE before any tracked run
    # without the call nothing changed: every rank holds the records of its own targets, their union is the one-rank log
    own = [res["engine/own"] for res in ranks]
    assert not {r[0] for r in own[0]} & {r[0] for r in own[1]} and all(len(o) > 0 for o in own)
    assert sorted(own[0] + own[1]) == single and len(single) > 0
    for res in ranks:
        assert res["engine/all"] == single and res["engine/all2"] == single
        assert res["engine/again"] == res["engine/stats"]
    assert [res["engine/stats"]["received"] for res in ranks] == [len(own[1]), len(own[0])]


def test_library_communicator_world_of_one():
    """fw_rejections_allgather_comm on the library's own RCCL communicator (one rank: ncclCommInitRank refuses two on one device)."""
    import flashweave_jl_amd as fw
    from flashweave_jl_amd import preprocess as pre, synth
    data, _, _ = pre.normalize(synth.generate(300, 250, 17, mode="S"), "fz")
    n, p = data.shape
    eng = fw.Engine("fz", n, p, max_k=3)
    try:
        eng.set_data(data)
        eng.compute_cor()
        with pytest.raises(fw.FlashWeaveError) as e:
            eng.gather_rejections_comm()  # no communicator
        assert e.value.code == -1
        eng.comm_init(fw.Engine.comm_unique_id(), 0, 1)
        eng.level0()
        eng.lgl_comm(feed_forward=True, round_size=32, track_rejections=True)
        before, c0 = eng.rejection_records().tobytes(), eng.comm_stats()["collectives"]
        assert len(before) > 0
        eng.gather_rejections_comm()
        c1 = eng.comm_stats()["collectives"]
        assert eng.rejection_records().tobytes() == before and c1 > c0
        eng.gather_rejections_comm()
        assert eng.rejection_records().tobytes() == before and eng.comm_stats()["collectives"] == c1
        eng.comm_destroy()
    finally:
        eng.close()


def test_two_records_for_one_slot_are_refused():
    """Targets are dealt to one rank each, so no two ranks send a record for one slot.  An exchange that hands rank 0's own block
    back as rank 1's as well breaks that: the unpack kernel sees the taken slots, the gather fails with FW_ERR_DEVICE and a message,
    and the log stays what it was -- no winner is picked."""
    import torch
    import flashweave_jl_amd as fw
    from flashweave_jl_amd import preprocess as pre, synth
    st = {}

    def prepare(user, n_local, aux_local, rec_bytes, d_send, d_recv, counts, aux, cap_records):
        n, st["log"] = int(n_local), rec_bytes == 96  # (24-byte records: the rounds of lgl, where rank 1 stays silent)
        st["bytes"] = max(n, 1) * rec_bytes
        st["send"] = torch.zeros(st["bytes"], dtype=torch.uint8, device="cuda:0")
        st["recv"] = torch.zeros(2 * st["bytes"], dtype=torch.uint8, device="cuda:0")
        counts[0], counts[1] = n, n if st["log"] else 0
        aux[0] = aux[1] = int(aux_local)
        d_send[0], d_recv[0], cap_records[0] = st["send"].data_ptr(), st["recv"].data_ptr(), max(n, 1)
        return 0

    def exchange(user):
        st["recv"][:st["bytes"]].copy_(st["send"])
        if st["log"]:
            st["recv"][st["bytes"]:].copy_(st["send"])
        torch.cuda.synchronize()
        return 0

    data, _, _ = pre.normalize(synth.generate(300, 250, 17, mode="S"), "fz")
    n, p = data.shape
    eng = fw.Engine("fz", n, p, max_k=3)
    try:
        eng.set_data(data)
        eng.compute_cor()
        eng.level0()
        eng.lgl(feed_forward=True, round_size=32, rank=0, world_size=2, dev_exchange=(prepare, exchange), track_rejections=True)
        before = eng.rejection_records().tobytes()
        assert len(before) > 0
        with pytest.raises(fw.FlashWeaveError, match="slot") as e:
            eng.gather_rejections((prepare, exchange))
        assert e.value.code == -2
        assert eng.rejection_records().tobytes() == before
    finally:
        eng.close()
