"""normalize_data(n_bins=, rank_method=, disc_method=) on the device: the binned kernels with their options (csrc/fw_norm.hip) against
the host front-end (preprocess.normalize), level for level -- dense and CSC, counts and abundances=True -- at the shapes where the
kernels take another path, the *_opts entry points at their defaults against the entry points without options and the reference's
fixtures, and normalize_data -> learn_network against the oracle.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import preprocess as pre
from oracle import oracle as O
from tests.norm_mode_tables import dense, fixture, hmp
from tests.util import load_norm, rel

pytestmark = pytest.mark.gpu
MODES = {"clr-nonzero-binned": {}, "tss-nonzero-binned": dict(norm="tss-nonzero-binned")}  # -> the norm keyword of the front-ends
OPTIONS = [dict(n_bins=b, rank_method=r) for b in (3, 4, 7) for r in ("tied", "dense")] + [dict(n_bins=3, disc_method="mean")]


def _ids(o):
    return "-".join(str(v) for v in o.values())


# ---- the tables ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tss_table():
    """300 x 24 counts, 40 % zeros, built for exact ties among the TSS quotients: few-valued counts (1 .. 4), 150 base samples, 100
    copies of base samples, and 50 samples that hold a base sample's counts in another column order (equal sums, shared counts)."""
    rng = np.random.default_rng(21)
    base = rng.integers(1, 5, size=(150, 24))
    base[rng.random(base.shape) < 0.4] = 0
    base[:, 0] = np.maximum(base[:, 0], 1)  # every sample has reads
    copies = base[rng.integers(0, 150, size=100)]
    shuffled = np.stack([base[i][rng.permutation(24)] for i in rng.integers(0, 150, size=50)])
    x = np.concatenate([base, copies, shuffled])[rng.permutation(300)]
    x.setflags(write=False)
    return x.astype(np.int64)


CLR_SEED = 0  # (the first seed at which clr_keys_are_apart holds for the table and for its real-valued form; the test asserts it)


@functools.lru_cache(maxsize=None)
def clr_table():
    """300 x 24 counts, 40 % zeros: 200 random base samples (counts up to 10^6) and 100 copies of base samples"""
    rng = np.random.default_rng(CLR_SEED)
    base = rng.integers(1, 10 ** 6, size=(200, 24))
    base[rng.random(base.shape) < 0.4] = 0
    base[:, 0] = np.maximum(base[:, 0], 1)
    x = np.concatenate([base, base[rng.integers(0, 200, size=100)]])[rng.permutation(300)]
    x.setflags(write=False)
    return x.astype(np.int64)


def real(x):
    """the table as real values that are no integers (abundances=True)"""
    return x.astype(np.float64) * 0.37


def clr_keys_are_apart(x):
    """The condition under which the ranks of the clr keys cannot hang on the last place of a log: within every column, two non-zero
    keys (the host's) either come from samples that are identical as whole rows, or differ by more than 1e-9 (1 + |key|) -- six
    orders above what a few ulps of log and of the row mean can move.  Identical rows give the same bits on either side."""
    data, _, _ = pre.filter_by_variance(np.asarray(x, dtype=np.float64))
    keys = pre.clr_nz(data)
    _, row_id = np.unique(data, axis=0, return_inverse=True)
    row_id = np.ravel(row_id)
    for j in range(data.shape[1]):
        nz = np.flatnonzero(data[:, j] != 0)
        order = nz[np.argsort(keys[nz, j], kind="stable")]
        k, r = keys[order, j], row_id[order]
        close = np.diff(k) <= 1e-9 * (1 + np.abs(k[:-1]))
        # sorted keys: a close pair that is not adjacent has a close adjacent pair between it; rows equal along a run of close keys
        if (close & (r[1:] != r[:-1])).any():
            return False
    return True


TABLES = {"clr-nonzero-binned": clr_table, "tss-nonzero-binned": tss_table}


@functools.lru_cache(maxsize=None)
def host(mode, kind, opts):
    """the host front-end's answer, computed once: (Int32 levels, row mask, column mask)"""
    x = TABLES[mode]()
    d, rm, cm = pre.normalize(real(x) if kind == "real" else x, "mi_nz", **MODES[mode], **dict(opts))
    return d.astype(np.int32), rm, cm


def same(got, exp, x, sparse=False):
    """(data, row_mask, col_mask) of a device front-end against the host's: masks, levels and -- sparse -- the CSC structure, one
    entry per present value of the kept block, rows ascending"""
    assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    assert sp.issparse(got[0]) is sparse and got[0].shape == exp[0].shape and got[0].dtype == np.int32
    assert np.array_equal(dense(got[0]), exp[0])
    if sparse:
        present = sp.csc_matrix(np.asarray(x)[exp[1]][:, exp[2]] != 0)
        present.sort_indices()
        assert np.array_equal(got[0].indptr, present.indptr) and np.array_equal(got[0].indices, present.indices)
        assert (got[0].data > 0).all()


def all_forms(x, exp, exp_real, **kw):
    """dense counts, CSC counts, dense abundances, CSC abundances against the host's answers"""
    same(fw.normalize_counts(x, "mi_nz", **kw), exp, x)
    same(fw.normalize_counts(sp.csc_matrix(x), "mi_nz", **kw), exp, x, sparse=True)
    if exp_real is not None:
        same(fw.normalize_abundances(real(x), "mi_nz", **kw), exp_real, x)
        same(fw.normalize_abundances(sp.csc_matrix(real(x)), "mi_nz", **kw), exp_real, x, sparse=True)


# ---- device == host -----------------------------------------------------------------------------------------------------------------
def test_the_tables_are_what_they_say():
    x = tss_table()
    assert x.shape == (300, 24) and 0.3 < (x == 0).mean() < 0.5 and len(np.unique(x, axis=0)) <= 200
    q = pre.tss(pre.filter_by_variance(x.astype(np.float64))[0])
    assert all(len(np.unique(q[x[:, j] != 0, j])) < (x[:, j] != 0).sum() // 2 for j in range(24))  # ties in every column
    y = clr_table()
    assert y.shape == (300, 24) and 0.3 < (y == 0).mean() < 0.5 and len(np.unique(y, axis=0)) == 200
    assert clr_keys_are_apart(y) and clr_keys_are_apart(real(y))
    # tied and dense ranks give different levels on the tied table (else the dense cases would show nothing)
    assert not np.array_equal(host("tss-nonzero-binned", "counts", (("n_bins", 4), ("rank_method", "tied")))[0],
                              host("tss-nonzero-binned", "counts", (("n_bins", 4), ("rank_method", "dense")))[0])


@pytest.mark.parametrize("opts", OPTIONS, ids=_ids)
@pytest.mark.parametrize("mode", sorted(MODES))
def test_device_front_ends_against_the_host(mode, opts):
    x, key = TABLES[mode](), tuple(sorted(opts.items()))
    exp, exp_real = host(mode, "counts", key), host(mode, "real", key)
    assert exp[0].shape[1] >= 12 and exp[0].max() == opts["n_bins"] - 1  # (most columns show all levels)
    all_forms(x, exp, exp_real, **MODES[mode], **opts)


# ---- shapes where the kernels take another path -------------------------------------------------------------------------------------
def _edge(x):
    """a TSS table (exact on either side) under the "mean" rule and at n_bins = 5 with dense and with tied ranks, counts dense and
    CSC, against the host -> the host's levels and column mask of the last"""
    for opts in (dict(disc_method="mean"), dict(n_bins=5, rank_method="dense"), dict(n_bins=5, rank_method="tied")):
        kw = dict(norm="tss-nonzero-binned", **opts)
        d, rm, cm = pre.normalize(x, "mi_nz", **kw)
        all_forms(x, (d.astype(np.int32), rm, cm), None, **kw)
    return d, cm


def _filled(n, p, seed, fill=0.6):
    """n x p counts in 1 .. 29, `fill` of them present, the last column full (every sample has reads; it is the longest column)"""
    rng = np.random.default_rng(seed)
    x = rng.integers(1, 30, size=(n, p))
    x[rng.random((n, p)) > fill] = 0
    x[:, -1] = rng.integers(1, 30, size=n)
    return x.astype(np.int64)


def test_one_non_zero_and_all_keys_equal():
    x = _filled(90, 6, 1)
    x[:, 0] = 0
    x[17, 0] = 5  # one non-zero entry: one key, one level
    x[:, 1] = 0
    x[40:, :] = 0
    x[40:, 1], x[40:, 5] = 3, 9  # fifty samples holding 3 of 12: fifty equal keys
    d, cm = _edge(x)
    assert not cm[0] and not cm[1] and cm[2:].all() and d.max() == 4


def test_padding_edge_1024_and_1025():
    x = _filled(1100, 4, 2, fill=1.0)
    x[1024:, 0] = 0  # 1 024 keys: the sort's power of two exactly
    x[1025:, 1] = 0  # 1 025: one key into the next
    d, cm = _edge(x)
    assert (x[:, 0] != 0).sum() == 1024 and (x[:, 1] != 0).sum() == 1025 and cm.all()


@pytest.mark.parametrize("n", [2048, 2049])
def test_csc_thread_switch(n):
    # the CSC kernel runs on 256 threads while the longest kept column pads to at most 2 048 keys, on 1 024 beyond
    x = _filled(n, 4, 3)
    assert max((x != 0).sum(axis=0)) == n
    _, cm = _edge(x)
    assert cm.all()


@pytest.mark.parametrize("n", [16384, 16385])
def test_keys_in_lds_and_in_device_memory(n):
    # 16 384 kept samples: the keys fill the LDS; 16 385: a slice of device memory per workgroup
    x = _filled(n, 6, 4)
    _, cm = _edge(x)
    assert cm.all()


def test_sixty_one_levels():
    rng = np.random.default_rng(6)
    x = np.zeros((200, 3), dtype=np.int64)
    x[:61, 0] = rng.permutation(61) + 1  # 61 distinct keys: every level once
    x[:, 1] = rng.permutation(200) + 1   # 200 distinct keys over 61 levels
    x[:, 2] = 1000 + np.arange(200) % 2
    x = x[rng.permutation(200)]
    for rank in ("tied", "dense"):
        kw = dict(norm="tss-nonzero-binned", n_bins=62, rank_method=rank)
        d, rm, cm = pre.normalize(x, "mi_nz", **kw)
        assert cm[:2].all() and sorted(d[d[:, 0] != 0, 0]) == list(range(1, 62)) and set(d[:, 1]) == set(range(1, 62))
        all_forms(x, (d.astype(np.int32), rm, cm), None, **kw)


# ---- the defaults through the new entry points --------------------------------------------------------------------------------------
def test_default_options_through_the_opts_entry_points():
    """The *_opts entry points with an explicit default struct (engine._opts_arg spells it out for them) give the bits of the entry
    points without options, and the reference's fixtures."""
    L, E = fw.load_library(), fw.engine
    x = hmp()
    xi, xf = np.asfortranarray(x.astype(np.int32)), np.asfortranarray(x.astype(np.float64))
    ci, cf = E.as_csc(sp.csc_matrix(x), np.int32), E.as_csc(sp.csc_matrix(x), np.float64)
    for test_name, norm, fx in (("mi_nz", None, load_norm("clr_nonzero_binned", np.int32)), ("mi_nz", "tss-nonzero-binned", fixture("tss-nonzero-binned")),
                                ("mi", None, load_norm("pres_abs", np.int32))):
        kw = {} if norm is None else dict(norm=norm)
        for old, new, table in ((L.fw_normalize_counts, L.fw_normalize_counts_opts, xi), (L.fw_normalize_abund, L.fw_normalize_abund_opts, xf)):
            a, b = E._normalize_dense(old, table, test_name, 0, **kw), E._normalize_dense(new, table, test_name, 0, **kw)
            assert all(np.array_equal(u, v) for u, v in zip(a, b)) and np.array_equal(b[0], fx) and b[0].dtype == np.int32
        for old, new, triple in ((L.fw_normalize_counts_csc, L.fw_normalize_counts_csc_opts, ci), (L.fw_normalize_abund_csc, L.fw_normalize_abund_csc_opts, cf)):
            a, b = E._normalize_csc(old, "test", triple, test_name, 0, **kw), E._normalize_csc(new, "test", triple, test_name, 0, **kw)
            assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(dense(b[0]), fx)
            assert all(np.array_equal(getattr(a[0], f), getattr(b[0], f)) for f in ("indptr", "indices", "data"))
    # the continuous kinds take the default struct as well
    a, b = E._normalize_dense(L.fw_normalize_counts, xi, "fz_nz", 0), E._normalize_dense(L.fw_normalize_counts_opts, xi, "fz_nz", 0)
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))


def test_the_entry_points_refuse_what_the_options_do_not_allow():
    """Past the Python refusals (the C ABI has other callers): FW_ERR_ARG with the field's name, dense and CSC."""
    L, E = fw.load_library(), fw.engine
    xi = np.asfortranarray(hmp().astype(np.int32))
    ci = E.as_csc(sp.csc_matrix(hmp()), np.int32)
    n, p = xi.shape
    out, rm, cm = np.zeros(n * p, np.int32), np.zeros(n, np.uint8), np.zeros(p, np.uint8)
    outf, ocp, orow = np.zeros(n * p, np.float32), np.zeros(p + 1, np.int64), np.zeros(n * p, np.int32)
    no, po, nz = E.C.c_int32(0), E.C.c_int32(0), E.C.c_int64(0)
    for kind, o, field in ((E.FW_MI_NZ, (2, 0, 0), "n_bins"), (E.FW_MI_NZ, (63, 0, 0), "n_bins"), (E.FW_NORM_TSS_BINNED, (3, 2, 0), "rank_method"),
                           (E.FW_MI_NZ, (3, 0, 7), "disc_method"), (E.FW_MI_NZ, (4, 0, 1), "disc_method"), (E.FW_FZ, (4, 0, 0), "n_bins"),
                           (E.FW_MI, (3, 1, 0), "rank_method"), (E.FW_NORM_TSS, (3, 0, 1), "disc_method")):
        opts = E.C.byref(E._NormOpts(*o))
        rc = L.fw_normalize_counts_opts(0, kind, n, p, E._ptr(xi), E._ptr(outf), E._ptr(out), E._ptr(rm), E._ptr(cm), E.C.byref(no), E.C.byref(po), opts)
        assert rc == -1 and field in L.fw_last_error(None).decode() and "fw_normalize_counts_opts" in L.fw_last_error(None).decode()
        rc = L.fw_normalize_counts_csc_opts(0, kind, n, p, E._ptr(ci.colptr), E._ptr(ci.rowval), E._ptr(ci.nzval), E._ptr(ocp), E._ptr(orow), E._ptr(out),
                                            E._ptr(outf), E._ptr(rm), E._ptr(cm), E.C.byref(no), E.C.byref(po), E.C.byref(nz), opts)
        assert rc == -1 and field in L.fw_last_error(None).decode()
    # a table none of whose columns shows all levels: the refusal names the number asked for
    with pytest.raises(fw.FlashWeaveError, match="61 non-zero levels"):
        fw.normalize_counts(hmp()[:40], "mi_nz", n_bins=62)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-12):
    return (a == b) or rel(a, b) < tol


def test_normalize_data_then_learn_network_against_the_oracle():
    """normalize_data(n_bins=4) -> learn_network(normalize=False): levels 0 .. 3 reach the engine's generic tables from the public
    entry point; levels and network against the oracle on the same matrix, as tests/test_gpu_mi.py::test_more_than_three_levels
    compares them (edge sets and integers exact, weights to 1e-12)."""
    rng = np.random.default_rng(12)
    lat = rng.standard_normal((700, 5))
    logits = lat @ rng.standard_normal((5, 40)) + 0.7 * rng.standard_normal((700, 40))
    counts = np.floor(np.exp(4.0 + 1.2 * logits)).astype(np.int64)
    counts[rng.random(counts.shape) < 0.3] = 0
    counts[:, 0] = np.maximum(counts[:, 0], 1)
    r = fw.normalize_data(counts, test_name="mi_nz", n_bins=4)
    rs = fw.normalize_data(sp.csc_matrix(counts), test_name="mi_nz", n_bins=4)
    data = r["data"]
    assert data.dtype == np.int32 and data.shape[1] >= 20 and data.max() == 3 and data.shape[0] == 700
    assert sp.issparse(rs["data"]) and np.array_equal(dense(rs["data"]), data) and rs["header"] == r["header"]
    on_host = fw.normalize_data(counts, test_name="mi_nz", n_bins=4, device_normalize=False)
    assert clr_keys_are_apart(counts) and on_host["header"] == r["header"] and np.array_equal(on_host["data"], data)
    orc = O.Oracle("mi_nz", np.ascontiguousarray(data), sparse=True, max_k=2)
    exp = orc.learn(max_k=2, feed_forward=True, round_size=1)
    assert max(orc.levels()[1]) == 3 and len(exp["edges"]) > 3
    for table in (data, rs["data"]):
        net = fw.learn_network(table, normalize=False, sensitive=False, heterogeneous=True, max_k=2, header=r["header"])
        assert set(net["edges"]) == set(exp["edges"])
        assert all(_close(net["edges"][e], w) for e, w in exp["edges"].items())
        assert net["parameters"]["test_name"] == "mi_nz" and net["variable_ids"] == r["header"]
