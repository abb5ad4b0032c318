"""CPU checks of the exact HITON-PC elimination mode (fast_elim = false, no_red_tests; fw_learn_opts.elim_mode).

The checker of the GPU tests (tests/test_gpu_exact_elim.py) is the Python restatement in tests/hiton_exact_ref.py.  Here it is
anchored: with fast_elim = True it equals Oracle.learn bit for bit on every kind, max_k and schedule the GPU tests use; and the
cases below show that exact mode (elim_mode 1) and elim_mode 2 really change results, so the GPU comparisons cannot pass vacuously."""
import numpy as np
import pytest

import flashweave_jl_amd as fw
from tests import hiton_exact_ref as H
from tests.hiton_exact_ref import make_oracles

SCHEDULES = [(True, 1), (True, 16), (False, 0)]  # (feed_forward, round_size): single_il, rounds of 16 with whitelists, ff = 0


@pytest.fixture(scope="module")
def oracles():
    return make_oracles()


def same_directed(a, b):
    return (np.array_equal(a["pc_off"], b["pc_off"]) and np.array_equal(a["pc_idx"], b["pc_idx"])
            and np.array_equal(a["pc_weight"], b["pc_weight"], equal_nan=True)
            and np.array_equal(a["pc_pval"], b["pc_pval"], equal_nan=True))


@pytest.mark.parametrize("kind", ["fz", "fz_nz", "mi", "mi_nz"])
@pytest.mark.parametrize("max_k", [1, 3, 5])
@pytest.mark.parametrize("ff,R", SCHEDULES)
def test_restatement_equals_oracle_in_fast_mode(oracles, kind, max_k, ff, R):
    orc, disc, _ = oracles[kind]
    got = H.learn(orc, disc, max_k=max_k, feed_forward=ff, round_size=R)
    exp = orc.learn(max_k=max_k, feed_forward=ff, round_size=R if R > 0 else 1)
    assert same_directed(got, exp)
    assert got["n_cond_tests"] == exp["n_cond_tests"] and got["edges"] == exp["edges"]
    assert got["n_cond_tests"] > 0


def test_restatement_equals_oracle_max_k_6_fz(oracles):
    orc, _, _ = oracles["fz"]
    got = H.learn(orc, False, max_k=6, feed_forward=True, round_size=1)
    exp = orc.learn(max_k=6, feed_forward=True, round_size=1)
    assert same_directed(got, exp) and got["n_cond_tests"] == exp["n_cond_tests"]


@pytest.mark.parametrize("kind", ["fz", "mi"])
@pytest.mark.parametrize("ff,R", SCHEDULES)
def test_exact_mode_changes_the_network(oracles, kind, ff, R):
    # a rejected member that stays in the pool can reject later members: fewer PC entries or other weights, and more tests
    orc, disc, _ = oracles[kind]
    fast = H.learn(orc, disc, max_k=3, feed_forward=ff, round_size=R)
    exact = H.learn(orc, disc, max_k=3, feed_forward=ff, round_size=R, fast_elim=False)
    assert not same_directed(fast, exact)
    assert exact["n_cond_tests"] > fast["n_cond_tests"]
    # no_red_tests = False has no effect with fast_elim = True (hiton.jl:388-390)
    assert same_directed(fast, H.learn(orc, disc, max_k=3, feed_forward=ff, round_size=R, no_red_tests=False))


@pytest.mark.parametrize("kind", ["fz_nz", "mi_nz"])
def test_elim_mode_2_keeps_elimination_statistics(oracles, kind):
    # update_PC_dict! skipped: PC keeps the elimination-phase statistics instead of the larger interleaving-phase p-values
    orc, disc, _ = oracles[kind]
    m1 = H.learn(orc, disc, max_k=3, feed_forward=False, round_size=0, fast_elim=False)
    m2 = H.learn(orc, disc, max_k=3, feed_forward=False, round_size=0, fast_elim=False, no_red_tests=False)
    assert np.array_equal(m1["pc_idx"], m2["pc_idx"]) and m1["n_cond_tests"] == m2["n_cond_tests"]
    assert not np.array_equal(m1["pc_pval"], m2["pc_pval"], equal_nan=True)
    assert (m2["pc_pval"] <= m1["pc_pval"]).all()  # update_PC_dict! only ever raises a p-value


def test_python_interface_takes_the_keywords():
    import inspect
    assert [f for f, _ in fw.engine._LearnOpts._fields_][-1] == "elim_mode"
    assert fw.engine.elim_mode(True, True) == 0 and fw.engine.elim_mode(True, False) == 0
    assert fw.engine.elim_mode(False, True) == 1 and fw.engine.elim_mode(False, False) == 2
    sig = inspect.signature(fw.learn_network).parameters
    assert sig["fast_elim"].default is True and sig["no_red_tests"].default is True  # learning.jl:207,469
    for m in (fw.Engine.lgl, fw.Engine.lgl_comm):
        ps = inspect.signature(m).parameters
        assert ps["fast_elim"].default is True and ps["no_red_tests"].default is True
