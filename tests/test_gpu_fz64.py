"""GPU tests of the Float64 Fisher-z mode (Engine(prec=64), learn_network(prec=64)) against the CPU oracle on its Float64 path,
mirroring tests/test_gpu_fz.py.

Tolerances:
  * Pearson matrix against oracle.cor(data, "f64"): the two differ in summation order only.  The dot product of two unit-norm
    centred columns carries at most gamma_n ~ n 2^-53 on either side (Cauchy-Schwarz on sum |x_i y_i|), plus a few ulps for
    the scaling: max |diff| <= 4 (n + 16) 2^-53 (1.4e-13 at n = 300; the Float32 path's own test allows 5e-6).
  * everything downstream, given the DEVICE's Float64 matrix: statistics bit-identical (only + - * / sqrt rint), p-values
    relative 1e-12 (device log / erfc vs libm).
  * golden networks through learn_network(prec=64): fixture print precision, 1e-7 (max_k 0) / 2e-7 (max_k 3)."""
import ctypes as C

import numpy as np
import pytest

import flashweave_jl_amd as fw
from flashweave_jl_amd import engine as E
from flashweave_jl_amd import io as fio
from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd import synth
from oracle import oracle as O
from tests import hiton_exact_ref as H
from tests import hiton_rej_ref as HR
from tests.util import GOLDEN, read_edgelist, rel

pytestmark = pytest.mark.gpu

FW_ERR_ARG, FW_ERR_STATE, FW_ERR_LIMIT = -1, -3, -5


def _cor_bound(n):
    return 4.0 * (n + 16) * 2.0 ** -53


def _synth_fz64(p, n, seed, **kw):
    counts = synth.generate(p, n, seed, mode="S", **kw)
    data, _, _ = pre.normalize(counts, "fz", prec=64)
    assert data.dtype == np.float64
    return np.asfortranarray(data)


@pytest.fixture(scope="module")
def small():
    data = _synth_fz64(400, 300, 11)
    n, p = data.shape
    eng = fw.Engine("fz", n, p, max_k=3, prec=64)
    eng.set_data(data)
    cm = eng.cor()
    orc = O.Oracle("fz", cor_mat=cm, n_obs=n)
    return dict(data=data, n=n, p=p, eng=eng, cm=cm, orc=orc)


def test_cor_matrix_is_float64_within_the_summation_bound(small):
    cm, data, n = small["cm"], small["data"], small["n"]
    assert cm.dtype == np.float64
    ref = O.cor(data, "f64")
    err = np.abs(cm - ref).max()
    print("fz64 cor: n = %d, max |diff| = %.3e, bound = %.3e" % (n, err, _cor_bound(n)))
    assert err <= _cor_bound(n)
    assert (cm == cm.T).all()                      # mirrored writes: exactly symmetric
    assert (np.diag(cm) == 1.0).all()
    assert np.abs(cm).max() <= 1.0


def test_cor_matrix_ragged_shapes():
    # n not a multiple of the k-tile (16), p not a multiple of the 128 tile nor of 4
    rng = np.random.default_rng(5)
    for n, p in ((37, 5), (100, 131), (333, 257)):
        data = np.asfortranarray(rng.standard_normal((n, p)))
        data[:, 0] = 1.5  # zero-variance column -> NaN row/col except the unit diagonal (Statistics.cor)
        eng = fw.Engine("fz", n, p, prec=64)
        eng.set_data(data)
        cm = eng.cor()
        ref = O.cor(data, "f64")
        assert cm.dtype == np.float64
        assert np.isnan(cm[0, 1:]).all() and np.isnan(cm[1:, 0]).all() and cm[0, 0] == 1.0
        err = np.abs(cm[1:, 1:] - ref[1:, 1:]).max()
        print("fz64 cor ragged: n = %d, p = %d, max |diff| = %.3e, bound = %.3e" % (n, p, err, _cor_bound(n)))
        assert err <= _cor_bound(n)
        assert (cm[1:, 1:] == cm[1:, 1:].T).all() and (np.diag(cm) == 1.0).all() and np.abs(cm[1:, 1:]).max() <= 1.0
        eng.close()


def test_single_tests_bit_exact(small):
    eng, orc, p = small["eng"], small["orc"], small["p"]
    rng = np.random.default_rng(3)
    X, Y, Zs = [], [], []
    for _ in range(3000):
        k = int(rng.integers(0, 6))
        v = rng.choice(p, size=k + 2, replace=False)
        X.append(int(v[0])); Y.append(int(v[1])); Zs.append(tuple(int(t) for t in v[2:]))
    # duplicated conditioning variables (feed-forward whitelist) and Z == X
    X += [1, 2, 3]; Y += [5, 6, 7]; Zs += [(9, 9), (11, 12, 11), (3, 8)]
    got = eng.test_batch(X, Y, Zs)
    for x, y, z, g in zip(X, Y, Zs, got):
        s, pv, df, pw = orc.test(x, y, z, n_obs_min=20)
        assert (g.stat == s) or (np.isnan(g.stat) and np.isnan(s)), (x, y, z, g.stat, s)
        assert rel(g.pval, pv) < 1e-12 or (np.isnan(g.pval) and np.isnan(pv))
        assert g.df == 0 and g.suff_power == pw


def _check_subsets(eng, orc, T, C_, A, max_k, alpha=0.01, max_tests=10_000_000):
    got = eng.test_subsets_batch(T, C_, A)
    for t, c, a, g in zip(T, C_, A, got):
        e = orc.test_subsets(t, c, a, max_k=max_k, alpha=alpha, n_obs_min=20, max_tests=max_tests)
        assert g["status"] == e["status"], (t, c, a, g, e)
        assert g["num_tests"] == e["num_tests"], (t, c, a, g, e)
        if e["status"] == 0:
            assert np.isnan(g["stat"]) and np.isnan(g["pval"]) and g["df"] == -1
            continue
        assert g["Zs"] == e["Zs"], (t, c, a, g, e)
        assert g["stat"] == e["stat"], (g, e)
        assert rel(g["pval"], e["pval"]) < 1e-12
        assert rel(g["frac"], e["frac"]) < 1e-12


def test_test_subsets_matches_reference_order(small):
    eng, orc, p = small["eng"], small["orc"], small["p"]
    rng = np.random.default_rng(4)
    T, C_, A = [], [], []
    for _ in range(400):
        a = int(rng.integers(0, 30))
        v = rng.choice(p, size=a + 2, replace=False)
        T.append(int(v[0])); C_.append(int(v[1])); A.append([int(t) for t in v[2:]])
    # jobs built from the strongest neighbours: long all-significant runs -> exercises the max-p rule
    cm = small["cm"]
    for t in range(20):
        order = np.argsort(-np.abs(cm[t]))
        nb = [int(v) for v in order if v != t][:14]
        T.append(t); C_.append(nb[0]); A.append(nb[1:])
    A[3] = A[3] + A[3][:1]  # duplicate in the accepted list
    _check_subsets(eng, orc, T, C_, A, max_k=3)


def test_test_subsets_max_tests_and_large_pool(small):
    n, p, cm, orc = small["n"], small["p"], small["cm"], small["orc"]
    eng = fw.Engine("fz", n, p, max_k=3, max_tests=37, prec=64)
    eng.set_cor_mat(cm)
    T, C_, A = [], [], []
    for t in range(30):
        order = np.argsort(-np.abs(cm[t]))
        nb = [int(v) for v in order if v != t][:12]
        T.append(t); C_.append(nb[0]); A.append(nb[1:])
    _check_subsets(eng, orc, T, C_, A, max_k=3, max_tests=37)
    eng.close()
    rng = np.random.default_rng(8)
    eng = fw.Engine("fz", n, p, max_k=2, max_tests=3000, alpha=0.9999, prec=64)
    eng.set_cor_mat(cm)
    big = [int(v) for v in rng.integers(2, p, size=2100)]
    _check_subsets(eng, orc, [0], [1], [big], max_k=2, alpha=0.9999, max_tests=3000)
    eng.close()


@pytest.mark.parametrize("max_k", [1, 2, 4, 5])
def test_test_subsets_other_max_k(small, max_k):
    n, p, cm, orc = small["n"], small["p"], small["cm"], small["orc"]
    eng = fw.Engine("fz", n, p, max_k=max_k, prec=64)
    eng.set_cor_mat(cm)
    T, C_, A = [], [], []
    for t in range(25):
        order = np.argsort(-np.abs(cm[t]))
        nb = [int(v) for v in order if v != t][:9]
        T.append(t); C_.append(nb[0]); A.append(nb[1:])
    _check_subsets(eng, orc, T, C_, A, max_k=max_k)
    eng.close()


def test_level0_neighbours(small):
    eng, orc = small["eng"], small["orc"]
    got = eng.pw_univar_neighbors()
    exp = orc.level0(alpha=0.01, n_obs_min=20)
    assert got["off"][-1] > 0
    assert (got["off"] == exp["off"]).all()
    assert (got["idx"] == exp["idx"]).all()
    assert (got["stat"] == exp["stat"]).all()
    assert np.allclose(got["pval"], exp["pval"], rtol=1e-12, atol=0)


@pytest.mark.parametrize("ff,R", [(False, 0), (True, 1), (True, 16), (True, 0), (False, 16)])
def test_network_matches_oracle(small, ff, R):
    n, p, cm, orc = small["n"], small["p"], small["cm"], small["orc"]
    eng = fw.Engine("fz", n, p, max_k=3, prec=64)
    eng.set_cor_mat(cm)
    got = eng.lgl(feed_forward=ff, round_size=R)
    exp = orc.learn(max_k=3, feed_forward=ff and R > 0, round_size=max(R, 1) if ff else 1)
    assert set(got["edges"]) == set(exp["edges"])
    for e, w in exp["edges"].items():
        assert got["edges"][e] == w            # weights are partial correlations: bit-exact
    assert np.array_equal(got["pc_off"], exp["pc_off"]) and np.array_equal(got["pc_idx"], exp["pc_idx"])
    assert np.array_equal(got["pc_weight"], exp["pc_weight"], equal_nan=True)
    cn = eng.counters()
    assert cn["cond_tests_ref"] == exp["n_cond_tests"]
    assert cn["level0_tests"] == p * (p - 1) // 2
    eng.close()


@pytest.fixture(scope="module")
def small80():
    # the table of tests/hiton_exact_ref.make_oracles, normalised to Float64; the checkers run on the device's Float64 matrix
    data = _synth_fz64(80, 300, 3, habitats=4)
    n, p = data.shape
    eng = fw.Engine("fz", n, p, max_k=3, prec=64)
    eng.set_data(data)
    cm = eng.cor()
    eng.close()
    return dict(data=data, n=n, p=p, cm=cm, orc=O.Oracle("fz", cor_mat=cm, n_obs=n))


@pytest.mark.parametrize("no_red_tests", [True, False])
def test_exact_elimination_matches_the_checker(small80, no_red_tests):
    c = small80
    eng = fw.Engine("fz", c["n"], c["p"], max_k=3, prec=64)
    eng.set_data(c["data"])
    got = eng.lgl(feed_forward=True, round_size=16, fast_elim=False, no_red_tests=no_red_tests)
    cnt = eng.counters()
    eng.close()
    exp = H.learn(c["orc"], False, max_k=3, feed_forward=True, round_size=16, fast_elim=False, no_red_tests=no_red_tests)
    assert np.array_equal(got["pc_off"], exp["pc_off"]) and np.array_equal(got["pc_idx"], exp["pc_idx"])
    assert cnt["cond_tests_ref"] == exp["n_cond_tests"]
    assert np.array_equal(got["pc_weight"], exp["pc_weight"], equal_nan=True)
    assert np.allclose(got["pc_pval"], exp["pc_pval"], rtol=1e-12, atol=0.0, equal_nan=True)


def test_track_rejections_matches_the_checker(small80):
    c = small80
    eng = fw.Engine("fz", c["n"], c["p"], max_k=3, prec=64)
    eng.set_data(c["data"])
    got = eng.lgl(feed_forward=True, round_size=1, track_rejections=True)
    plain = eng.lgl(feed_forward=True, round_size=1)
    eng.close()
    assert got["edges"] == plain["edges"]  # the log is a diagnostic mode: same network
    exp = HR.learn(c["orc"], False, max_k=3, feed_forward=True, round_size=1)
    assert np.array_equal(got["pc_idx"], exp["pc_idx"]) and np.array_equal(got["pc_weight"], exp["pc_weight"], equal_nan=True)
    want = {(T, cd): r for T, d in exp["rejections"].items() for cd, r in d.items()}
    rec = got["rejection_records"]
    have = {(int(r["target"]), int(r["candidate"])): r for r in rec}
    assert len(have) == len(rec) and len(want) > 0
    assert set(have) == set(want)
    for k, w in want.items():
        g = have[k]
        assert tuple(int(v) for v in g["zs"][:int(g["n_zs"])]) == w["Zs"], k
        assert int(g["num_tests"]) == w["num_tests"] and int(g["df"]) == w["df"], (k, g, w)
        assert bool(g["suff_power"]) == w["suff_power"] and int(g["phase"]) == w["phase"], (k, g, w)
        assert int(g["n_acc"]) == len(w["pool"]), (k, g, w)
        assert float(g["frac"]) == w["frac"], (k, float(g["frac"]), w["frac"])
        assert float(g["stat"]) == w["stat"], (k, float(g["stat"]), w["stat"])
        assert np.isclose(float(g["pval"]), w["pval"], rtol=1e-12, atol=0.0), (k, float(g["pval"]), w["pval"])


@pytest.mark.parametrize("max_k,n_edges,wtol", [(0, 60, 1e-7), (3, 50, 2e-7)])
def test_learn_network_prec64_reproduces_the_golden_networks(max_k, n_edges, wtol):
    # reference test/learning.jl:522-531: exp_fz_maxk{0,3}.edgelist were generated with prec=64; p = 50 -> single_il
    raw, header, _ = fio.read_table(GOLDEN + "/HMP_SRA_gut_small.tsv")
    net = fw.learn_network(raw, sensitive=True, heterogeneous=False, max_k=max_k, prec=64)
    assert net["parameters"]["prec"] == 64 and net["parameters"]["round_size"] == 1
    assert not net["counters"]["normalized_on_device"]
    exp = read_edgelist("%s/learning_expected/exp_fz_maxk%d.edgelist" % (GOLDEN, max_k))
    assert len(exp) == n_edges
    assert set(net["edges"]) == set(exp)
    worst = max(abs(net["edges"][e] - exp[e]) for e in exp)
    print("fz64 golden max_k=%d: max |weight diff| = %.3e" % (max_k, worst))
    assert worst <= wtol
    # an already normalised Float64 matrix with normalize=False takes the same path
    data, _, _ = pre.normalize(raw, "fz", prec=64)
    net2 = fw.learn_network(data, max_k=max_k, prec=64, normalize=False)
    assert net2["edges"] == net["edges"]
    # fz_nz keeps Float32 values whatever prec says, and says so
    nz = fw.learn_network(raw, sensitive=True, heterogeneous=True, max_k=max_k, prec=64)
    assert nz["parameters"]["prec"] == 32


def _err(eng, rc, code, *words):
    msg = eng.L.fw_last_error(eng.h).decode()
    assert rc == code, (rc, code, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_precisions_never_mix():
    n, p = 64, 8
    rng = np.random.default_rng(1)
    d64 = np.asfortranarray(rng.standard_normal((n, p)))
    d32 = np.asfortranarray(d64.astype(np.float32))
    o64, o32 = np.zeros((p, p), np.float64, order="F"), np.zeros((p, p), np.float32, order="F")
    ptr = E._ptr
    # a Float32 context refuses the Float64 getter, and the Float64 setters once it holds Float32 input
    e32 = fw.Engine("fz", n, p)
    e32.set_data(d32)
    e32.cor()
    _err(e32, e32.L.fw_get_cor_mat_f64(e32.h, ptr(o64)), FW_ERR_STATE, "fw_get_cor_mat_f64", "not in Float64 mode")
    _err(e32, e32.L.fw_set_data_dense_f64(e32.h, ptr(d64)), FW_ERR_STATE, "fw_set_data_dense_f64", "Float32 input")
    _err(e32, e32.L.fw_set_cor_mat_f64(e32.h, ptr(o64)), FW_ERR_STATE, "fw_set_cor_mat_f64", "Float32 input")
    assert e32.cor_mat().dtype == np.float32  # and goes on working
    e32.close()
    # a Float64 context refuses the Float32 getter and setters
    e64 = fw.Engine("fz", n, p, prec=64)
    e64.set_data(d64)
    cm = e64.cor()
    assert cm.dtype == np.float64
    _err(e64, e64.L.fw_get_cor_mat(e64.h, ptr(o32)), FW_ERR_STATE, "fw_get_cor_mat", "Float64 mode")
    _err(e64, e64.L.fw_set_data_dense_f32(e64.h, ptr(d32)), FW_ERR_STATE, "fw_set_data_dense_f32", "Float64 mode")
    _err(e64, e64.L.fw_set_cor_mat(e64.h, ptr(o32)), FW_ERR_STATE, "fw_set_cor_mat", "Float64 mode")
    assert np.array_equal(e64.cor_mat(), cm)
    # ... and the sharded / communicator entry points, each by name
    L, h = e64.L, e64.h
    a, b = C.c_int64(0), C.c_int64(0)
    opts = E._LearnOpts(1, 1, 0, 1, 0, 0)
    _err(e64, L.fw_compute_cor_mat_rows(h, 0, 1, C.byref(a), C.byref(b)), FW_ERR_LIMIT, "fw_compute_cor_mat_rows", "Float64 mode")
    _err(e64, L.fw_use_cor_buffer(h, C.c_void_p(0), 0), FW_ERR_LIMIT, "fw_use_cor_buffer", "Float64 mode")
    _err(e64, L.fw_level0_sharded(h, 0, 1, None, None, C.byref(a)), FW_ERR_LIMIT, "fw_level0_sharded", "Float64 mode")
    _err(e64, L.fw_level0_sharded_dev(h, 0, 1, None, C.byref(a)), FW_ERR_LIMIT, "fw_level0_sharded_dev", "Float64 mode")
    _err(e64, L.fw_learn_network_dev(h, C.byref(opts), None, C.byref(a)), FW_ERR_LIMIT, "fw_learn_network_dev", "Float64 mode")
    buf = (C.c_uint8 * 128)()
    _err(e64, L.fw_comm_init(h, buf, 0, 1), FW_ERR_LIMIT, "fw_comm_init", "Float64 mode")
    _err(e64, L.fw_level0_comm(h, C.byref(a)), FW_ERR_LIMIT, "fw_level0_comm", "Float64 mode")
    _err(e64, L.fw_learn_network_comm(h, C.byref(opts), C.byref(a)), FW_ERR_LIMIT, "fw_learn_network_comm", "Float64 mode")
    _err(e64, L.fw_cor_mat_allgather_comm(h, 128), FW_ERR_LIMIT, "fw_cor_mat_allgather_comm", "Float64 mode")
    e64.close()
    # the Float64 setters on another test kind
    for kind, data in (("fz_nz", d32), ("mi", (d32 > 0).astype(np.int32))):
        e = fw.Engine(kind, n, p)
        _err(e, e.L.fw_set_data_dense_f64(e.h, ptr(d64)), FW_ERR_ARG, "fw_set_data_dense_f64", "not FW_FZ")
        _err(e, e.L.fw_set_cor_mat_f64(e.h, ptr(o64)), FW_ERR_ARG, "fw_set_cor_mat_f64", "not FW_FZ")
        e.close()
    # options the Float64 mode does not serve, each by name (the context stays a Float32 one)
    for kw, word in ((dict(recursive_pcor=False), "recursive_pcor = 0"), (dict(recursive_pcor=False, dense_cor=False), "no_cor_mat = 1"),
                     (dict(max_k=6), "max_k = 6"), (dict(max_k=7), "max_k = 7")):
        e = fw.Engine("fz", n, p, **kw)
        _err(e, e.L.fw_set_data_dense_f64(e.h, ptr(d64)), FW_ERR_LIMIT, "fw_set_data_dense_f64", word)
        _err(e, e.L.fw_set_cor_mat_f64(e.h, ptr(np.asfortranarray(cm))), FW_ERR_LIMIT, "fw_set_cor_mat_f64", word)
        e.set_data(d32)
        e.close()
    # more than five conditioning variables in a single test
    e = fw.Engine("fz", n, p, max_k=3, prec=64)
    e.set_cor_mat(cm)
    with pytest.raises(fw.FlashWeaveError, match="Float64 mode serves up to 5"):
        e.test(0, 1, (2, 3, 4, 5, 6, 7))
    e.close()
