"""GPU tests of the exact HITON-PC elimination mode (learn_network(fast_elim=False), no_red_tests=False; fw_learn_opts.elim_mode)
against the Python restatement of the driver (tests/hiton_exact_ref.py, anchored to the CPU oracle in test_exact_elim_cpu.py).

Every path the library has for it: the host job pool (FW_HOST_HITON=1, single_il rounds, max_k 6), the device rounds of fz / fz_nz
(fw_devhiton.hip, FW_DEV_MIN_TARGETS=1), the persistent discrete kernel's device schedule (FW_DEV_MIN_TARGETS=1) and its per-round
loop (FW_MI_SCHED=0).  Integers (directed lists, reference-order test counts) must match exactly; fz statistics bit for bit (the
restatement is fed the device's Float32 matrix); discrete statistics within the tolerances of test_gpu_mi.py."""
import ctypes as C

import numpy as np
import pytest

import flashweave_jl_amd as fw
from flashweave_jl_amd import engine as E
from oracle import oracle as O
from tests import hiton_exact_ref as H
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

SCHEDULES = [(True, 1), (True, 16), (False, 0)]
PATHS = {"default": {}, "host": {"FW_HOST_HITON": "1"}, "dev": {"FW_DEV_MIN_TARGETS": "1"},
         "rounds": {"FW_DEV_MIN_TARGETS": "1", "FW_MI_SCHED": "0"}}
MODES = [(False, True), (False, False)]  # elim_mode 1, 2


@pytest.fixture(scope="module")
def ctx():
    out = {}
    for kind, (orc, disc, data) in H.make_oracles().items():
        n, p = data.shape
        if kind == "fz":  # the restatement runs on the device's own Float32 matrix
            eng = fw.Engine("fz", n, p, max_k=3)
            eng.set_data(data)
            eng.compute_cor()
            orc = O.Oracle("fz", cor_mat=np.asfortranarray(eng.cor()), n_obs=n)
            eng.close()
        out[kind] = dict(orc=orc, disc=disc, data=data, n=n, p=p, ref={})
    return out


def _ref(c, max_k, ff, R, fast_elim, no_red_tests):
    key = (max_k, ff, R, fast_elim, no_red_tests)
    if key not in c["ref"]:
        c["ref"][key] = H.learn(c["orc"], c["disc"], max_k=max_k, feed_forward=ff, round_size=R, fast_elim=fast_elim,
                                no_red_tests=no_red_tests)
    return c["ref"][key]


def _run(kind, c, max_k, ff, R, env, monkeypatch, **kw):
    for k in ("FW_HOST_HITON", "FW_DEV_MIN_TARGETS", "FW_MI_SCHED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = fw.Engine(kind, c["n"], c["p"], max_k=max_k)
    try:
        eng.set_data(c["data"])
        if kind == "fz":
            eng.compute_cor()
        net = eng.lgl(feed_forward=ff, round_size=R, **kw)
        return net, eng.counters()
    finally:
        eng.close()


def _check(kind, got, cnt, exp):
    assert np.array_equal(got["pc_off"], exp["pc_off"]) and np.array_equal(got["pc_idx"], exp["pc_idx"])
    assert cnt["cond_tests_ref"] == exp["n_cond_tests"]
    if kind in ("fz", "fz_nz"):
        assert np.array_equal(got["pc_weight"], exp["pc_weight"], equal_nan=True)
        assert np.allclose(got["pc_pval"], exp["pc_pval"], rtol=1e-12, atol=0.0, equal_nan=True)
    else:
        assert np.allclose(got["pc_weight"], exp["pc_weight"], rtol=1e-12, atol=1e-15, equal_nan=True)
        assert np.allclose(got["pc_pval"], exp["pc_pval"], rtol=1e-10, atol=0.0, equal_nan=True)


@pytest.mark.parametrize("kind", ["fz", "fz_nz", "mi", "mi_nz"])
@pytest.mark.parametrize("max_k", [1, 3, 5])
@pytest.mark.parametrize("ff,R", SCHEDULES)
@pytest.mark.parametrize("fast_elim,no_red_tests", MODES)
def test_every_path_equals_the_restatement(ctx, kind, max_k, ff, R, fast_elim, no_red_tests, monkeypatch):
    c = ctx[kind]
    exp = _ref(c, max_k, ff, R, fast_elim, no_red_tests)
    paths = ["default", "host", "dev"] + (["rounds"] if kind in ("mi", "mi_nz") else [])
    res = {}
    for name in paths:
        net, cnt = _run(kind, c, max_k, ff, R, PATHS[name], monkeypatch, fast_elim=fast_elim, no_red_tests=no_red_tests)
        _check(kind, net, cnt, exp)
        res[name] = net
    # the paths agree among themselves: the same bytes for fz / fz_nz; discrete host pool vs persistent kernel: the same integers, the
    # statistics to 1e-12 (one test per wavefront vs four: another summation order)
    first = res[paths[0]]
    for name in paths[1:]:
        for key in ("pc_off", "pc_idx") + (("pc_weight", "pc_pval") if kind in ("fz", "fz_nz") else ()):
            assert first[key].tobytes() == res[name][key].tobytes(), (name, key)


def test_fz_max_k_6_host_pool(ctx, monkeypatch):
    c = ctx["fz"]
    for fast_elim, no_red_tests in MODES:
        exp = _ref(c, 6, True, 1, fast_elim, no_red_tests)
        net, cnt = _run("fz", c, 6, True, 1, {}, monkeypatch, fast_elim=fast_elim, no_red_tests=no_red_tests)
        _check("fz", net, cnt, exp)


def test_default_mode_unchanged(ctx, monkeypatch):
    # elim_mode 0 is still the oracle's fast_elim network
    c = ctx["mi"]
    net, cnt = _run("mi", c, 3, True, 16, PATHS["dev"], monkeypatch)
    exp = c["orc"].learn(max_k=3, feed_forward=True, round_size=16)
    assert np.array_equal(net["pc_idx"], exp["pc_idx"]) and cnt["cond_tests_ref"] == exp["n_cond_tests"]


@pytest.mark.parametrize("kind", ["mi", "mi_nz"])
def test_discrete_device_schedule_is_deterministic(ctx, kind, monkeypatch):
    c = ctx[kind]
    runs = [_run(kind, c, 3, True, 16, PATHS["dev"], monkeypatch, fast_elim=False)[0] for _ in range(2)]
    for key in ("pc_off", "pc_idx", "pc_weight", "pc_pval", "edge_src", "edge_dst", "edge_weight"):
        if key in runs[0]:
            assert runs[0][key].tobytes() == runs[1][key].tobytes(), key
    assert runs[0]["edges"] == runs[1]["edges"]


def test_elim_mode_out_of_range_is_refused(ctx):
    c = ctx["mi"]
    eng = fw.Engine("mi", c["n"], c["p"], max_k=3)
    try:
        eng.set_data(c["data"])
        ne = C.c_int64(0)
        for bad in (3, -1):
            opts = E._LearnOpts(1, 1, 0, 1, 0, bad)
            with pytest.raises(fw.FlashWeaveError) as ei:
                eng._ck(eng.L.fw_learn_network(eng.h, C.byref(opts), None, None, C.byref(ne)))
            assert ei.value.code == -1  # FW_ERR_ARG
    finally:
        eng.close()


def test_reference_smoke_fast_elim_false():
    # the reference's "fast_elim" testset (test/learning.jl:385-389), with the result checked against the restatement
    raw = np.loadtxt(GOLDEN + "/HMP_SRA_gut_small.tsv", delimiter="\t", skiprows=1, usecols=range(1, 51))
    res = fw.learn_network(raw, sensitive=True, heterogeneous=False, max_k=3, fast_elim=False)
    assert isinstance(res, fw.FWResult)
    assert res["parameters"]["fast_elim"] is False and res["parameters"]["no_red_tests"] is True
    mat, _, col_mask = fw.normalize_counts(raw, "fz")  # what learn_network normalised with (integral table: on the device)
    n, p = mat.shape
    eng = fw.Engine("fz", n, p, max_k=3)
    try:
        eng.set_data(mat)
        eng.compute_cor()
        orc = O.Oracle("fz", cor_mat=np.asfortranarray(eng.cor()), n_obs=n)
    finally:
        eng.close()
    exp = H.learn(orc, False, max_k=3, feed_forward=True, round_size=fw.api.default_round_size(p), fast_elim=False)
    assert res["edges"] == exp["edges"] and len(exp["edges"]) > 0
    fast = fw.learn_network(raw, sensitive=True, heterogeneous=False, max_k=3)
    assert fast["parameters"]["fast_elim"] is True
