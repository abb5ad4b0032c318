"""The Fisher-z feed-forward schedule on the device (fwi_devhiton_fz_schedule, FW_FZ_SCHED=1: whitelists built and sorted on the device,
one download at the end) against the round loop with the host in between (FW_FZ_SCHED=0) and the oracle.  Everything the two drivers
hand back must be equal to the bit: edges, directed lists, statistics, p-values, reference-order test counts and job counts.

Which driver ran is read off the launch counter.  Both drivers count four kernels per round of the segment kernel; the schedule also
launches, and counts, dh_fz_init_kernel and dh_sched_pack_kernel once and dh_fz_round_begin_kernel once per chain and round of targets
(plus the local-matrix and whitelist-append kernels where they run), none of which the round loop has.
"""
import numpy as np
import pytest

import flashweave_jl_amd as fw
from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd import synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu

KEYS = ("pc_off", "pc_idx", "pc_weight", "pc_pval")


@pytest.fixture(scope="module")
def small():
    counts = synth.generate(400, 300, 11, mode="S")
    data, _, _ = pre.normalize(counts, "fz", prec=32)
    data = np.asfortranarray(data)
    n, p = data.shape
    eng = fw.Engine("fz", n, p, max_k=3)
    eng.set_data(data)
    cm = eng.cor()
    eng.close()
    return dict(n=n, p=p, cm=cm, orc=O.Oracle("fz", cor_mat=cm, n_obs=n))


def _extra_launches(cn):
    return cn["kernel_launches"] - 4 * cn["subsets_launches"]


def _schedule_ran(cs, cl, chain_rounds, ff):
    """init + pack + one round-begin kernel per chain and round, at most two more per chain and round; with feed-forward every chain
    and round but the last round's appends to the whitelists."""
    extra = _extra_launches(cs) - _extra_launches(cl)
    return 2 + chain_rounds + (chain_rounds // 2 if ff else 0) <= extra <= 2 + 3 * chain_rounds


def _run(make_engine, monkeypatch, sched, **lgl):
    """Two lgl calls on one engine under FW_FZ_SCHED=sched: (network, counters of the second call); the calls must agree to the byte
    (whitelist counts, target records or control state left over from the first call would show here)."""
    monkeypatch.setenv("FW_FZ_SCHED", sched)
    eng = make_engine()
    first = eng.lgl(**lgl)
    eng.reset_counters()
    net = eng.lgl(**lgl)
    cn = eng.counters()
    eng.close()
    assert first["edges"] == net["edges"]
    for key in KEYS:
        assert first[key].tobytes() == net[key].tobytes(), key
    return net, cn


def _both(make_engine, monkeypatch, **lgl):
    ns, cs = _run(make_engine, monkeypatch, "1", **lgl)
    nl, cl = _run(make_engine, monkeypatch, "0", **lgl)
    assert ns["edges"] == nl["edges"]
    for key in KEYS:
        assert np.array_equal(ns[key], nl[key], equal_nan=True), key
    assert cs["cond_tests_ref"] == cl["cond_tests_ref"] and cs["subsets_calls"] == cl["subsets_calls"]
    assert cs["subsets_launches"] > 0 and cl["subsets_launches"] > 0
    return ns, cs, cl


def _from_cm(small, max_k):
    def make():
        eng = fw.Engine("fz", small["n"], small["p"], max_k=max_k)
        eng.set_cor_mat(small["cm"])
        return eng
    return make


def _check_oracle(small, net, cn, ff, R):
    exp = small["orc"].learn(max_k=3, feed_forward=ff, round_size=max(R, 1) if ff else 1)
    assert set(net["edges"]) == set(exp["edges"])
    for e, w in exp["edges"].items():
        assert net["edges"][e] == w
    assert cn["cond_tests_ref"] == exp["n_cond_tests"]


# (True, 100): four rounds of two chains of 50; (True, 80): five rounds on one chain; (False, 0): one round, two chains of 200
@pytest.mark.parametrize("ff,R,chain_rounds", [(True, 100, 8), (True, 80, 5), (False, 0, 2)])
def test_schedule_equals_round_loop_and_oracle(small, ff, R, chain_rounds, monkeypatch):
    net, cs, cl = _both(_from_cm(small, 3), monkeypatch, feed_forward=ff, round_size=R)
    assert _schedule_ran(cs, cl, chain_rounds, ff)
    _check_oracle(small, net, cs, ff, R)


def test_schedule_max_k5(small, monkeypatch):
    _, cs, cl = _both(_from_cm(small, 5), monkeypatch, feed_forward=True, round_size=100)
    assert _schedule_ran(cs, cl, 8, True)


def test_schedule_exact_elimination(small, monkeypatch):
    _, cs, cl = _both(_from_cm(small, 3), monkeypatch, feed_forward=True, round_size=100, fast_elim=False)
    assert _schedule_ran(cs, cl, 8, True)


def test_schedule_long_whitelists_and_lists_past_the_table_limit(monkeypatch):
    # one shared factor (tests/test_gpu_fz.py: test_device_rounds_long_accepted_lists): every PC set holds nearly every variable, so
    # from the second round on the whitelists are hundreds of entries long and the accepted lists pass FW_TAB_A = 512 -- the bound that
    # switches the in-lane kernel on (accepted + whitelisted to come) starts from the longest DEVICE-built whitelist; a wrong word
    # there fails the call with "met a batch without the in-lane kernel"
    rng = np.random.default_rng(7)
    n, p = 2000, 600
    data = (rng.standard_normal((n, 1)) + 0.9 * rng.standard_normal((n, p))).astype(np.float32)

    def make():
        eng = fw.Engine("fz", n, p, max_k=3, max_tests=300)
        eng.set_data(data)
        eng.cor()
        return eng

    net, cs, cl = _both(make, monkeypatch, feed_forward=True, round_size=150)
    assert np.diff(net["pc_off"]).max() > 512
    assert _schedule_ran(cs, cl, 8, True)


def test_last_round_below_the_threshold_keeps_the_round_loop(small, monkeypatch):
    # rounds of 64 on 400 targets: the last one holds 16, which the round loop gives to the host pool -> no schedule, same network
    net, cs, cl = _both(_from_cm(small, 3), monkeypatch, feed_forward=True, round_size=64)
    assert _extra_launches(cs) == _extra_launches(cl)
    _check_oracle(small, net, cs, True, 64)
