"""GPU tests of the rejection log (learn_network(track_rejections=True); fw_set_track_rejections / fw_rejections_count /
fw_rejections_get) against the Python restatement of the driver with the rejection branch (tests/hiton_rej_ref.py, anchored to the
CPU oracle in tests/test_rejections_cpu.py).

Every path the library has: the host job pool (FW_HOST_HITON=1, single_il rounds, max_k 6), the device rounds of fz / fz_nz
(FW_DEV_MIN_TARGETS=1), the persistent discrete kernel's device schedule (FW_DEV_MIN_TARGETS=1) and its per-round loop
(FW_MI_SCHED=0).  The record SET must equal the checker's: target, candidate, Zs (order included), num_tests, df, suff_power, phase
and frac exactly; stat / pval under the tolerances tests/test_gpu_exact_elim.py uses for pc_weight / pc_pval."""
import ctypes as C

import numpy as np
import pytest

import flashweave_jl_amd as fw
from flashweave_jl_amd import io as fio
from oracle import oracle as O
from tests import hiton_rej_ref as HR
from tests.util import GOLDEN, load_norm, read_edgelist

pytestmark = pytest.mark.gpu

SCHEDULES = [(True, 1), (True, 16), (False, 0)]
PATHS = {"default": {}, "host": {"FW_HOST_HITON": "1"}, "dev": {"FW_DEV_MIN_TARGETS": "1"},
         "rounds": {"FW_DEV_MIN_TARGETS": "1", "FW_MI_SCHED": "0"}}
KINDS = ["fz", "fz_nz", "mi", "mi_nz"]


def _paths(kind):
    return ["default", "host", "dev"] + (["rounds"] if kind in ("mi", "mi_nz") else [])


def _context(**kw):
    out = {}
    for kind, (orc, disc, data) in HR.make_oracles(**kw).items():
        n, p = data.shape
        if kind == "fz":  # the restatement runs on the device's own Float32 matrix
            eng = fw.Engine("fz", n, p, max_k=3)
            eng.set_data(data)
            eng.compute_cor()
            orc = O.Oracle("fz", cor_mat=np.asfortranarray(eng.cor()), n_obs=n)
            eng.close()
        out[kind] = dict(orc=orc, disc=disc, data=data, n=n, p=p, ref={})
    return out


@pytest.fixture(scope="module")
def ctx():
    return _context()


@pytest.fixture(scope="module")
def ctx300():
    return _context(p=300, n=600)


def _ref(c, max_k, ff, R, fast_elim=True, no_red_tests=True):
    key = (max_k, ff, R, fast_elim, no_red_tests)
    if key not in c["ref"]:
        c["ref"][key] = HR.learn(c["orc"], c["disc"], max_k=max_k, feed_forward=ff, round_size=R, fast_elim=fast_elim,
                                 no_red_tests=no_red_tests)
    return c["ref"][key]


def _run(kind, c, max_k, ff, R, env, monkeypatch, track=True, **kw):
    for k in ("FW_HOST_HITON", "FW_DEV_MIN_TARGETS", "FW_MI_SCHED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = fw.Engine(kind, c["n"], c["p"], max_k=max_k)
    try:
        eng.set_data(c["data"])
        if kind == "fz":
            eng.compute_cor()
        net = eng.lgl(feed_forward=ff, round_size=R, track_rejections=track, **kw)
        return net, eng.counters()
    finally:
        eng.close()


def _check_records(kind, rec, exp, tag):
    """rec: structured array of fw_rejection; exp: the checker's {T: {cand: record}}."""
    want = {(T, cd): r for T, d in exp.items() for cd, r in d.items()}
    got = {(int(r["target"]), int(r["candidate"])): r for r in rec}
    print(tag, "records", len(rec), "expected", len(want))
    assert len(got) == len(rec), (tag, "duplicate (target, candidate)")
    assert set(got) == set(want), (tag, len(got), len(want), sorted(set(got) ^ set(want))[:8])
    keys = [(int(r["target"]), int(r["candidate"])) for r in rec]
    assert keys == sorted(keys), (tag, "records are not in ascending (target, candidate) order")
    for k, w in want.items():
        g = got[k]
        zs = tuple(int(v) for v in g["zs"][:int(g["n_zs"])])
        assert zs == w["Zs"], (tag, k, zs, w["Zs"])
        assert int(g["num_tests"]) == w["num_tests"] and int(g["df"]) == w["df"], (tag, k, g, w)
        assert bool(g["suff_power"]) == w["suff_power"] and int(g["phase"]) == w["phase"], (tag, k, g, w)
        assert int(g["n_acc"]) == len(w["pool"]), (tag, k, g, w)
        assert float(g["frac"]) == w["frac"], (tag, k, float(g["frac"]), w["frac"])
        if kind in ("fz", "fz_nz"):
            assert float(g["stat"]) == w["stat"], (tag, k, float(g["stat"]), w["stat"])
            assert np.isclose(float(g["pval"]), w["pval"], rtol=1e-12, atol=0.0), (tag, k, float(g["pval"]), w["pval"])
        else:
            assert np.isclose(float(g["stat"]), w["stat"], rtol=1e-12, atol=1e-15), (tag, k, float(g["stat"]), w["stat"])
            assert np.isclose(float(g["pval"]), w["pval"], rtol=1e-10, atol=0.0), (tag, k, float(g["pval"]), w["pval"])


def _check_net(kind, got, cnt, exp):
    assert np.array_equal(got["pc_off"], exp["pc_off"]) and np.array_equal(got["pc_idx"], exp["pc_idx"])
    assert cnt["cond_tests_ref"] == exp["n_cond_tests"]


MODES = [(True, True), (False, True)]  # elim_mode 0, 1 (elim_mode 2: once per kind below)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("max_k", [1, 3, 5])
@pytest.mark.parametrize("ff,R", SCHEDULES)
@pytest.mark.parametrize("fast_elim,no_red_tests", MODES)
def test_every_path_returns_the_checkers_records(ctx, kind, max_k, ff, R, fast_elim, no_red_tests, monkeypatch):
    c = ctx[kind]
    exp = _ref(c, max_k, ff, R, fast_elim, no_red_tests)
    for name in _paths(kind):
        net, cnt = _run(kind, c, max_k, ff, R, PATHS[name], monkeypatch, fast_elim=fast_elim, no_red_tests=no_red_tests)
        _check_net(kind, net, cnt, exp)
        _check_records(kind, net["rejection_records"], exp["rejections"], (kind, max_k, ff, R, fast_elim, name))


@pytest.mark.parametrize("kind", KINDS)
def test_elim_mode_2(ctx, kind, monkeypatch):
    c = ctx[kind]
    exp = _ref(c, 3, True, 16, False, False)
    for name in _paths(kind):
        net, cnt = _run(kind, c, 3, True, 16, PATHS[name], monkeypatch, fast_elim=False, no_red_tests=False)
        _check_net(kind, net, cnt, exp)
        _check_records(kind, net["rejection_records"], exp["rejections"], (kind, "elim_mode 2", name))


def test_fz_max_k_6_host_pool(ctx, monkeypatch):
    c = ctx["fz"]
    for fast_elim in (True, False):
        exp = _ref(c, 6, True, 1, fast_elim, True)
        net, cnt = _run("fz", c, 6, True, 1, {}, monkeypatch, fast_elim=fast_elim)
        _check_net("fz", net, cnt, exp)
        _check_records("fz", net["rejection_records"], exp["rejections"], ("fz", 6, fast_elim))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fast_elim", [True, False])
def test_p300_table_every_path(ctx300, kind, fast_elim, monkeypatch):
    # stops far beyond the first window of a job (tests/test_rejections_cpu.py asserts how far on this table)
    c = ctx300[kind]
    exp = _ref(c, 3, True, 16, fast_elim, True)
    for name in _paths(kind):
        net, cnt = _run(kind, c, 3, True, 16, PATHS[name], monkeypatch, fast_elim=fast_elim)
        _check_net(kind, net, cnt, exp)
        _check_records(kind, net["rejection_records"], exp["rejections"], (kind, "p300", fast_elim, name))


NET_KEYS = ("pc_off", "pc_idx", "pc_weight", "pc_pval", "edge_src", "edge_dst", "edge_weight")


@pytest.mark.parametrize("kind", KINDS)
def test_tracking_changes_nothing_and_is_deterministic(ctx, kind, monkeypatch):
    c = ctx[kind]
    for name in _paths(kind):
        for fast_elim in (True, False):
            off, cnt0 = _run(kind, c, 3, True, 16, PATHS[name], monkeypatch, track=False, fast_elim=fast_elim)
            on1, cnt1 = _run(kind, c, 3, True, 16, PATHS[name], monkeypatch, fast_elim=fast_elim)
            on2, _ = _run(kind, c, 3, True, 16, PATHS[name], monkeypatch, fast_elim=fast_elim)
            assert off["rejections"] == {} and "rejection_records" not in off
            for key in NET_KEYS:
                assert off[key].tobytes() == on1[key].tobytes(), (kind, name, fast_elim, key)
            assert off["edges"] == on1["edges"] and cnt0["cond_tests_ref"] == cnt1["cond_tests_ref"]
            assert len(on1["rejection_records"]) > 0
            assert on1["rejection_records"].tobytes() == on2["rejection_records"].tobytes(), (kind, name, fast_elim)


def test_log_state(ctx):
    c = ctx["mi"]
    eng = fw.Engine("mi", c["n"], c["p"], max_k=3)
    try:
        eng.set_data(c["data"])
        n = C.c_int64(-1)
        assert eng.L.fw_rejections_count(eng.h, C.byref(n)) == -3  # FW_ERR_STATE: no tracked run yet
        with pytest.raises(fw.FlashWeaveError) as ei:
            eng.rejection_records()
        assert ei.value.code == -3
        eng.lgl(feed_forward=True, round_size=16)  # untracked: still no log
        assert eng.L.fw_rejections_count(eng.h, C.byref(n)) == -3
        net = eng.lgl(feed_forward=True, round_size=16, track_rejections=True)
        assert len(net["rejection_records"]) > 0 and len(eng.rejection_records()) == len(net["rejection_records"])
        eng.lgl(feed_forward=True, round_size=16)  # untracked run after a tracked one: empty, not stale
        assert eng.L.fw_rejections_count(eng.h, C.byref(n)) == 0 and n.value == 0
        assert len(eng.rejection_records()) == 0
    finally:
        eng.close()


def test_learn_network_golden_table_with_track_rejections(tmp_path):
    # reference test/learning.jl:290-310: learn_network(..., track_rejections=true) on the bundled table still gives the expected
    # networks, and the log is there and survives the reference's file format
    raw, header, _ = fio.read_table(GOLDEN + "/HMP_SRA_gut_small.tsv")
    for sensitive, het, name, wtol in ((True, False, "fz", 5e-5), (True, True, "fz_nz", 2e-5),
                                       (False, False, "mi", 1e-13), (False, True, "mi_nz", 1e-13)):
        net = fw.learn_network(raw, sensitive=sensitive, heterogeneous=het, max_k=3, track_rejections=True)
        assert net["parameters"]["track_rejections"] is True
        exp = read_edgelist("%s/learning_expected/exp_%s_maxk3.edgelist" % (GOLDEN, name))
        assert set(net["edges"]) == set(exp), name
        assert all(abs(net["edges"][e] - exp[e]) <= wtol for e in exp)
        rej = net["rejections"]
        if name in ("mi", "mi_nz"):
            # the discrete modes against the checker on the bundled normalised tables.  mi_nz: exp_mi_nz_maxk3 is the EMPTY network --
            # no variable has a univariate neighbour on this table, so no candidate is ever tested and the reference's log is empty
            # as well (accepted + rejected = the univariate neighbours); the log must then be empty, not merely "there"
            fx = load_norm("pres_abs" if name == "mi" else "clr_nonzero_binned", np.int64)
            chk = HR.learn(O.Oracle(name, np.ascontiguousarray(fx), sparse=True, max_k=3), True, max_k=3, feed_forward=True, round_size=1)
            assert {T: {c: (r["Zs"], r["df"], r["suff_power"], r["num_tests"], r["frac"]) for c, r in d.items()} for T, d in chk["rejections"].items()} == \
                   {T: {c: (v[0], v[1][2], v[1][3], v[2][0], v[2][1]) for c, v in d.items()} for T, d in rej.items()}, name
            assert (len(rej) > 0) == (len(exp) > 0), name
        else:
            assert sum(len(d) for d in rej.values()) > 0, name
        plain = fw.learn_network(raw, sensitive=sensitive, heterogeneous=het, max_k=3)
        assert plain["edges"] == net["edges"] and plain["rejections"] == {} and plain["parameters"]["track_rejections"] is False
        path = str(tmp_path / ("rej_%s.tsv" % name))
        net.save_rejections(path)
        back = fio.load_rejections(path)
        assert set(back) == set(rej)
        for T in rej:
            assert set(back[T]) == set(rej[T])
            for cd, (zs, (stat, pval, df, pw), (nt, frac)) in rej[T].items():
                bzs, (bstat, bpval, bdf, bpw), (bnt, bfrac) = back[T][cd]
                assert (bzs, bdf, bpw, bnt) == (zs, df, pw, nt)
                assert abs(bstat - stat) <= 0.5e-5 + 1e-12 and abs(bpval - pval) <= 0.5e-5 + 1e-12 and abs(bfrac - frac) <= 0.5e-5 + 1e-12
