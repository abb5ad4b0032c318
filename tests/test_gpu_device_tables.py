"""Tables that already live in GPU memory (a torch.Tensor with device.type "cuda"): Engine.set_data, normalize_counts /
normalize_abundances, normalize_data and learn_network take them without a host copy (fw_set_data_dense_*_dev, fw_normalize_*_dev).
Everything is compared with what the same table gives as a numpy array, and every comparison is exact: the resident layouts and the
front-end's bits are the same by construction, so nothing is left to a tolerance."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import flashweave_jl_amd as fw
from flashweave_jl_amd import synth
from tests.norm_mode_tables import bits, edge_table

pytestmark = pytest.mark.gpu
GPU = "cuda:0"
N_GRID = (63, 64, 65, 130)  # plane-word edges and a ragged last word
P_GRID = (5, 129)  # within and across one level-0 tile of 128 variables
FORMS = ("row_major", "col_major", "int64")


def as_tensor(x, form="row_major"):
    """the numpy table in GPU memory: contiguous as torch lays it out, with strides (1, n), or widened to int64 / float64"""
    if form == "col_major":
        t = torch.from_numpy(np.ascontiguousarray(x.T)).to(GPU).t()
        assert tuple(t.shape) == x.shape and t.stride() == (1, x.shape[0])
        return t
    t = torch.from_numpy(np.ascontiguousarray(x)).to(GPU)
    assert t.stride() == (x.shape[1], 1)
    return t.to(torch.int64 if x.dtype.kind == "i" else torch.float64) if form == "int64" else t


def discrete_table(n, p, top):
    """values 0 .. min(top, 2) that follow three hidden columns (so that level 0 and the network are not empty); column 1 is all
    zero, column 2 holds no zero; top == 3: a single 3 in the last row of the last column, the switch to the generic form"""
    rng = np.random.default_rng(1000 * n + 10 * p + top)
    hi = min(top, 2)
    hidden = rng.integers(0, hi + 1, size=(n, 3))
    x = np.where(rng.random((n, p)) < 0.75, hidden[:, np.arange(p) % 3], rng.integers(0, hi + 1, size=(n, p))).astype(np.int32)
    x[:, 1] = 0
    x[:, 2] = 1 + np.arange(n) % hi
    if top == 3:
        x[n - 1, p - 1] = 3
    return x


def jobs(p, max_k=2, m=36):
    """a few dozen fixed (X, Y, Zs), conditioning sets of 0 .. max_k variables"""
    rng = np.random.default_rng(7)
    X, Y, Zs = [], [], []
    for t in range(m):
        v = rng.permutation(p)[:2 + max_k]
        X.append(int(v[0])), Y.append(int(v[1])), Zs.append(tuple(int(q) for q in v[2:2 + t % (max_k + 1)]))
    return X, Y, Zs


def result_bits(results):
    return [(bits(np.float64(r.stat)).item(), bits(np.float64(r.pval)).item(), r.df, r.suff_power) for r in results]


def edge_bits(edges):
    return {e: bits(np.float64(w)).item() for e, w in edges.items()}


def engine_state(kind, table, **kw):
    """what an engine holds and computes after set_data(table), in a form that compares to the bit; kw: Engine's keywords"""
    n, p = table.shape
    auto = fw.Engine(kind, n, p, max_k=2)  # the automatic n_obs_min follows the levels of the upload
    auto.set_data(table)
    out = dict(n_obs_min=auto.n_obs_min)
    if kind in ("mi", "mi_nz"):
        out["levels"], out["max_vals"] = (a.tolist() for a in auto.levels())
    auto.close()
    eng = fw.Engine(kind, n, p, max_k=2, n_obs_min=10, **kw)
    eng.set_data(table)
    if kind == "fz":
        out["cor"] = bits(eng.cor()).tolist()
    l0 = eng.pw_univar_neighbors()
    out["l0"] = (l0["off"].tolist(), l0["idx"].tolist(), bits(l0["stat"]).tolist(), bits(l0["pval"]).tolist())
    out["tests"] = result_bits(eng.test_batch(*jobs(p)))
    out["edges"] = edge_bits(eng.lgl()["edges"])
    eng.close()
    return out


@functools.lru_cache(maxsize=None)
def discrete_reference(kind, n, p, top):
    """the numpy upload of discrete_table(n, p, top), computed once"""
    return engine_state(kind, discrete_table(n, p, top))


# ---- layout build, discrete ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("top", [1, 2, 3])
@pytest.mark.parametrize("p", P_GRID)
@pytest.mark.parametrize("n", N_GRID)
@pytest.mark.parametrize("kind", ["mi", "mi_nz"])
def test_discrete_layout_built_on_the_device(kind, n, p, top, form):
    x = discrete_table(n, p, top)
    assert x.max() == top and not x[:, 1].any() and x[:, 2].all()
    exp = discrete_reference(kind, n, p, top)
    assert exp["levels"][1] == 1 and exp["levels"][2] == min(top, 2) and max(exp["max_vals"]) == top
    got = engine_state(kind, as_tensor(x, form))
    assert got.keys() == exp.keys()
    for key in exp:
        assert got[key] == exp[key], key
    if n == 130 and p == 129:
        assert len(exp["l0"][1]) > 0 and len(exp["edges"]) > 0  # (the comparison is not one of empty lists)


# ---- layout build, continuous ----------------------------------------------------------------------------------------------------
def continuous_table(n, p, zeros):
    """Float64 values that follow three hidden columns; zeros: 40 % absences, one of them a -0.0, and one stored value that rounds
    to 0.0f as a Float32"""
    rng = np.random.default_rng(2000 * n + p)
    hidden = rng.standard_normal((n, 3))
    x = hidden[:, np.arange(p) % 3] + 0.7 * rng.standard_normal((n, p))
    if zeros:
        x[rng.random((n, p)) < 0.4] = 0.0
        x[3, 0], x[5, p - 1] = -0.0, 1e-60
        assert np.float32(x[5, p - 1]) == 0.0 and np.signbit(x[3, 0])
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("p", P_GRID)
@pytest.mark.parametrize("n", N_GRID)
def test_fz_nz_plane_built_on_the_device(n, p, dtype):
    x = continuous_table(n, p, zeros=True).astype(dtype)
    exp = engine_state("fz_nz", x)
    for form in ("row_major", "col_major"):
        got = engine_state("fz_nz", as_tensor(x, form))
        for key in exp:
            assert got[key] == exp[key], (form, key)
    if n == 130 and p == 129:
        assert len(exp["l0"][1]) > 0 and len(exp["edges"]) > 0


@pytest.mark.parametrize("n,p", [(65, 5), (130, 129)])
def test_fz_matrix_copied_on_the_device(n, p):
    x = continuous_table(n, p, zeros=False).astype(np.float32)
    exp = engine_state("fz", x)
    for form in ("row_major", "col_major", "int64"):  # ("int64": widened to Float64, converted back on the device)
        got = engine_state("fz", as_tensor(x, form))
        for key in exp:
            assert got[key] == exp[key], (form, key)
    assert p < 129 or len(exp["edges"]) > 0


# ---- refusals: the host path's code and message, and the context stays usable ---------------------------------------------------
def refusal(call):
    """(code, text) of the FlashWeaveError a call raises, None when it passes"""
    try:
        call()
    except fw.FlashWeaveError as e:
        return e.code, str(e)
    return None


def good_upload_follows(eng, kind, n, p):
    """eng: made with n_obs_min=10 (the automatic one is beyond these n, and level 0 would say so)"""
    x = discrete_table(n, p, 2)
    eng.set_data(as_tensor(x))
    assert [a.tolist() for a in eng.levels()] == [discrete_reference(kind, n, p, 2)[k] for k in ("levels", "max_vals")]
    eng.pw_univar_neighbors()


@pytest.mark.parametrize("kind", ["mi", "mi_nz"])
def test_a_value_out_of_range_is_refused_as_the_host_refuses_it(kind):
    n, p = 65, 5
    for cells in ({(10, 3): 62, (30, 3): 70, (2, 4): -1},  # the lowest bad column, the value at its first bad row
                  {(64, 2): -1, (0, 4): 62},
                  {(0, 0): 2 ** 31 - 1}):
        x = discrete_table(n, p, 2)
        for (i, j), v in cells.items():
            x[i, j] = v
        host, dev = fw.Engine(kind, n, p, max_k=2, n_obs_min=10), fw.Engine(kind, n, p, max_k=2, n_obs_min=10)
        exp = refusal(lambda: host.set_data(x))
        (i, j), v = sorted(cells.items(), key=lambda c: (c[0][1], c[0][0]))[0]
        assert exp is not None and exp[0] == -5 and "column %d holds %d" % (j, v) in exp[1]
        for form in FORMS:
            assert refusal(lambda: dev.set_data(as_tensor(x, form))) == exp, form
        good_upload_follows(dev, kind, n, p)
        host.close(), dev.close()


def test_limits_of_the_discrete_tables_are_the_host_path_s():
    n, p = 65, 5
    big = discrete_table(n, p, 2)
    big[7, 3] = 61  # 62 levels: the table of a test with five conditioning variables is beyond the device-memory limit
    for kind, table, max_k in (("mi", discrete_table(n, p, 2), 7), ("mi_nz", big, 5)):
        host, dev = fw.Engine(kind, n, p, max_k=max_k), fw.Engine(kind, n, p, max_k=max_k)
        exp = refusal(lambda: host.set_data(table))
        assert exp is not None and exp[0] == -5
        assert refusal(lambda: dev.set_data(as_tensor(table))) == exp
        ok = discrete_table(n, p, 1)  # two levels fit either limit
        host.set_data(ok), dev.set_data(as_tensor(ok))
        assert [a.tolist() for a in dev.levels()] == [a.tolist() for a in host.levels()]
        host.close(), dev.close()


def test_null_and_host_pointers_are_refused_without_a_dereference():
    L = fw.load_library()
    n, p = 65, 5
    mi, fz = fw.Engine("mi", n, p, max_k=2, n_obs_min=10), fw.Engine("fz_nz", n, p, max_k=2)
    host_i, host_f = np.zeros((p, n), np.int32), np.zeros((p, n), np.float32)
    assert L.fw_set_data_dense_i32_dev(mi.h, None) == -1 and b"NULL" in L.fw_last_error(mi.h)
    assert L.fw_set_data_dense_f32_dev(fz.h, None) == -1 and b"NULL" in L.fw_last_error(fz.h)
    assert L.fw_set_data_dense_i32_dev(mi.h, host_i.ctypes.data_as(ctypes.c_void_p)) == -1 and b"not device memory" in L.fw_last_error(mi.h)
    assert L.fw_set_data_dense_f32_dev(fz.h, host_f.ctypes.data_as(ctypes.c_void_p)) == -1 and b"not device memory" in L.fw_last_error(fz.h)
    rm, cm, no, po = np.zeros(n, np.uint8), np.zeros(p, np.uint8), ctypes.c_int32(0), ctypes.c_int32(0)
    out = torch.empty(n * p, dtype=torch.int32, device=GPU)
    table = as_tensor(discrete_table(n, p, 2), "col_major")
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for front_end in (L.fw_normalize_counts_dev, L.fw_normalize_abund_dev):
        tail = (vp(rm), vp(cm), ctypes.byref(no), ctypes.byref(po), None)
        assert front_end(0, fw.FW_MI, n, p, None, None, ctypes.c_void_p(out.data_ptr()), *tail) == -1
        assert front_end(0, fw.FW_MI, n, p, vp(host_i), None, ctypes.c_void_p(out.data_ptr()), *tail) == -1
        assert b"not device memory" in L.fw_last_error(None)
        assert front_end(0, fw.FW_MI, n, p, ctypes.c_void_p(table.data_ptr()), None, vp(host_i), *tail) == -1
        assert b"output buffer is not device memory" in L.fw_last_error(None)
    good_upload_follows(mi, "mi", n, p)
    mi.close(), fz.close()


# ---- front-end -----------------------------------------------------------------------------------------------------------------
def count_table(which):
    """300 x 24 (the generator of tests/norm_mode_tables.py) or 65 x 5: a constant column and empty samples are filtered out"""
    return edge_table(300, 24) if which == "300x24" else edge_table()[:65, :6][:, 1:]


def real_table(which):
    y = count_table(which).astype(np.float64) * 0.37
    y[:, 5 if which == "300x24" else 4] = 0.5  # (a dyadic constant)
    return y


FRONT_END = ([dict(norm_mode=m) for m in ("clr-adapt", "clr-nonzero", "clr-nonzero-binned", "pres-abs", "tss", "tss-nonzero-binned")] +
             [dict(test_name="mi_nz", n_bins=b, rank_method=r) for b in (3, 4) for r in ("tied", "dense")] +
             [dict(norm_mode="tss-nonzero-binned", n_bins=4, rank_method="dense"), dict(test_name="mi_nz", disc_method="mean"),
              dict(norm_mode="tss-nonzero-binned", disc_method="mean")])


def same_normalized(got, exp, n, p):
    assert isinstance(got["data"], torch.Tensor) and got["data"].is_cuda
    data = got["data"].cpu().numpy()
    assert data.dtype == exp["data"].dtype and data.shape == exp["data"].shape and got["data"].stride() == (1, data.shape[0])
    assert np.array_equal(bits(data), bits(exp["data"]))
    assert got["header"] == exp["header"] and np.array_equal(got["row_mask"], exp["row_mask"])
    assert np.array_equal(got["meta_mask"], exp["meta_mask"])
    assert data.shape[0] < n and data.shape[1] < p  # a sample and a column were filtered out


@pytest.mark.parametrize("which", ["300x24", "65x5"])
@pytest.mark.parametrize("kw", FRONT_END, ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_front_end_on_a_device_tensor(kw, which):
    x = count_table(which)
    header = ["otu%d" % j for j in range(x.shape[1])]
    exp = fw.normalize_data(x, header=header, **kw)
    for form in FORMS:
        same_normalized(fw.normalize_data(as_tensor(x, form), header=header, **kw), exp, *x.shape)


@pytest.mark.parametrize("which", ["300x24", "65x5"])
@pytest.mark.parametrize("kw", [dict(test_name="fz"), dict(test_name="fz_nz"), dict(test_name="mi"), dict(test_name="mi_nz"),
                                dict(norm_mode="tss"), dict(norm_mode="tss-nonzero-binned", n_bins=4)],
                         ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_front_end_on_a_real_valued_device_tensor(kw, which):
    y = real_table(which)
    exp = fw.normalize_data(y, abundances=True, **kw)
    for form in ("row_major", "col_major"):
        same_normalized(fw.normalize_data(as_tensor(y, form), abundances=True, **kw), exp, *y.shape)
    same_normalized(fw.normalize_data(as_tensor(y.astype(np.float32)), abundances=True, **kw),
                    fw.normalize_data(y.astype(np.float32), abundances=True, **kw), *y.shape)


def test_engine_level_front_ends_return_a_view_of_the_output_buffer():
    x = count_table("300x24")
    got, exp = fw.normalize_counts(as_tensor(x), "mi_nz"), fw.normalize_counts(x, "mi_nz")
    assert got[0].is_cuda and got[0].stride() == (1, got[0].shape[0]) and np.array_equal(got[0].cpu().numpy(), exp[0])
    assert all(isinstance(m, np.ndarray) and np.array_equal(m, e) for m, e in zip(got[1:], exp[1:]))
    with pytest.raises(TypeError, match="integer counts"):
        fw.normalize_counts(as_tensor(x * 0.5), "mi_nz")
    with pytest.raises(ValueError, match=r"\[0, 2\^31 - 1\]"):
        fw.normalize_counts(as_tensor(x - 1), "mi_nz")
    with pytest.raises(ValueError, match="a negative value"):
        fw.normalize_abundances(as_tensor(x - 1.0), "fz")
    with pytest.raises(ValueError, match="outside"):
        fw.normalize_abundances(as_tensor(x * 2.0 ** 100), "fz", norm="tss")


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def synth_counts():
    return synth.generate(40, 200, seed=5)


@pytest.mark.parametrize("test_name", ["fz", "fz_nz", "mi", "mi_nz"])
def test_learn_network_on_a_device_tensor(test_name):
    counts = synth_counts()
    assert counts.shape == (200, 40)
    kw = dict(sensitive=test_name.startswith("fz"), heterogeneous=test_name.endswith("_nz"), track_rejections=test_name == "fz", max_k=2)
    exp, got = fw.learn_network(counts, **kw), fw.learn_network(as_tensor(counts), **kw)
    assert edge_bits(got["edges"]) == edge_bits(exp["edges"]) and len(exp["edges"]) > 0
    assert got["variable_ids"] == exp["variable_ids"] and got["meta_variable_mask"] == exp["meta_variable_mask"]
    assert got["rejections"] == exp["rejections"] and (test_name != "fz" or len(exp["rejections"]) > 0)
    assert got["counters"]["table_on_device"] is True and got["parameters"]["table_on_device"] is True
    assert "table_on_device" not in exp["counters"] and "table_on_device" not in exp["parameters"]
    assert {k: v for k, v in got["parameters"].items() if k != "table_on_device"} == exp["parameters"]
    assert got["counters"]["normalized_on_device"] and set(got["counters"]) - set(exp["counters"]) == {"table_on_device"}


@pytest.mark.parametrize("test_name", ["fz", "mi_nz"])
def test_normalize_data_then_learn_network_stays_on_the_device(test_name):
    counts = synth_counts()
    kw = dict(sensitive=test_name == "fz", heterogeneous=test_name == "mi_nz", max_k=2)
    r = fw.normalize_data(as_tensor(counts), test_name=test_name)
    assert r["data"].is_cuda
    got = fw.learn_network(r["data"], normalize=False, header=r["header"], **kw)
    exp = fw.learn_network(counts, **kw)
    assert edge_bits(got["edges"]) == edge_bits(exp["edges"]) and got["variable_ids"] == exp["variable_ids"]
    assert got["parameters"]["table_on_device"] is True


# ---- what a device tensor is not served with --------------------------------------------------------------------------------------
def test_every_refusal_names_its_option_and_the_way_out(monkeypatch):
    counts = synth_counts()
    t = as_tensor(counts)
    called = []
    monkeypatch.setattr(fw.api, "normalize_counts", lambda *a, **k: called.append("normalize_counts"))
    monkeypatch.setattr(fw.api, "normalize_abundances", lambda *a, **k: called.append("normalize_abundances"))
    monkeypatch.setattr(fw.api, "Engine", lambda *a, **k: called.append("Engine"))
    meta = np.arange(200.0).reshape(200, 1)
    both = [(dict(meta_data=meta), "meta_data"), (dict(meta_mask=np.arange(40) == 0), "meta_mask"),
            (dict(extra_data=[(counts, None)]), "extra_data"), (dict(prec=64), "prec=64"),
            (dict(device_normalize=False), "device_normalize=False")]
    for entry in (fw.learn_network, fw.normalize_data):
        for kw, name in both:
            with pytest.raises(ValueError, match=r"%s with a table in GPU memory.*tensor\.cpu\(\)" % name):
                entry(t, **kw)
        with pytest.raises(ValueError, match=r"abundances=True.*tensor\.cpu\(\)"):
            entry(as_tensor(counts * 0.5))
        with pytest.raises(ValueError, match=r"device=1 .*tensor\.cpu\(\)"):
            entry(t, device=1)
        for bad in (t[0], t[None], t.to(torch.complex64)):
            with pytest.raises(ValueError, match=r"2-D.*numeric dtype.*tensor\.cpu\(\)"):
                entry(bad)
        with pytest.raises(ValueError, match=r"sparse torch tensor.*tensor\.cpu\(\)"):
            entry(t.to_sparse())
    with pytest.raises(ValueError, match=r"distributed=True with a table in GPU memory.*tensor\.cpu\(\)"):
        fw.learn_network(t, distributed=True)
    with pytest.raises(ValueError, match=r"csc_resident=True with a table in GPU memory.*tensor\.cpu\(\)"):
        fw.learn_network(t, sensitive=True, heterogeneous=True, csc_resident=True)
    assert called == []  # before any library call
    eng = fw.Engine("fz", 200, 40, prec=64)
    with pytest.raises(ValueError, match="prec=64"):
        eng.set_data(as_tensor(counts.astype(np.float64)))
    eng.close()
    eng = fw.Engine("fz_nz", 200, 40)
    with pytest.raises(ValueError, match="csc_resident=True"):
        eng.set_data(as_tensor(counts.astype(np.float32)), csc_resident=True)
    with pytest.raises(ValueError, match="sparse torch tensor"):
        eng.set_data(as_tensor(counts.astype(np.float32)).to_sparse())
    eng.close()
