"""Sparse tables that already live in GPU memory (a torch.Tensor with layout torch.sparse_csc and device.type "cuda"): Engine.set_data,
normalize_counts / normalize_abundances, normalize_data and learn_network take them without a host trip (fw_set_data_csc_*_dev,
fw_normalize_*_csc_dev).  Everything is compared with what the same table gives as a scipy.sparse.csc_matrix on the same build -- a
path the oracle and the goldens pin -- and every comparison is exact, floats as bit patterns: the resident layouts and the front-end's
bits are the same by construction, so nothing is left to a tolerance.  The tensors are built with torch.sparse_csc_tensor over the
scipy arrays moved to the GPU."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import flashweave_jl_amd as fw
from tests.csc_device_tables import N_GRID, P_GRID, TOPS, count_csc, discrete_csc, fznz_csc
from tests.norm_mode_tables import bits
from tests.test_gpu_device_tables import edge_bits, jobs, refusal, result_bits

pytestmark = pytest.mark.gpu
GPU = "cuda:0"
INDEX_DTYPES = (torch.int64, torch.int32)


def csc_tensor(m, index=torch.int64, values=None):
    """the scipy CSC matrix as a sparse CSC tensor in GPU memory: its three arrays as they are (no invariant check, nothing sorted),
    both index arrays of dtype `index`"""
    data = m.data if values is None else values
    return torch.sparse_csc_tensor(torch.from_numpy(m.indptr).to(GPU).to(index), torch.from_numpy(m.indices).to(GPU).to(index),
                                   torch.from_numpy(np.ascontiguousarray(data)).to(GPU), size=m.shape)


def engine_state(kind, table, csc_resident=False, max_k=2, **kw):
    """what tests/test_gpu_device_tables.py's engine_state compares -- n_obs_min, levels, max_vals, the level-0 lists, a few dozen
    test_batch results and lgl's edges, to the bit -- plus data_resident_bytes() for fz_nz, after set_data(table, csc_resident)"""
    n, p = table.shape
    auto = fw.Engine(kind, n, p, max_k=max_k)  # the automatic n_obs_min follows the levels of the upload
    auto.set_data(table, csc_resident=csc_resident)
    out = dict(n_obs_min=auto.n_obs_min)
    if kind in ("mi", "mi_nz"):
        out["levels"], out["max_vals"] = (a.tolist() for a in auto.levels())
    auto.close()
    eng = fw.Engine(kind, n, p, max_k=max_k, n_obs_min=10, **kw)
    eng.set_data(table, csc_resident=csc_resident)
    if kind == "fz_nz":
        out["resident_bytes"] = eng.data_resident_bytes()
    l0 = eng.pw_univar_neighbors()
    out["l0"] = (l0["off"].tolist(), l0["idx"].tolist(), bits(l0["stat"]).tolist(), bits(l0["pval"]).tolist())
    out["tests"] = result_bits(eng.test_batch(*jobs(p, max_k)))
    out["edges"] = edge_bits(eng.lgl()["edges"])
    eng.close()
    return out


def max_k_of(top):
    """conditioning sets of two variables, of one at 62 levels: a test's table is L^max_k (L^2 + 1) words, and 62^2 x 3 845 of them per
    wavefront make a case take most of a minute where 62 x 3 845 take a second; the layout under test is the same"""
    return 2 if top < 61 else 1


@functools.lru_cache(maxsize=None)
def discrete_reference(kind, n, p, top):
    """the scipy upload of discrete_csc(n, p, top), computed once"""
    return engine_state(kind, discrete_csc(n, p, top), max_k=max_k_of(top))


# ---- layout build, discrete ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("top", TOPS)
@pytest.mark.parametrize("p", P_GRID)
@pytest.mark.parametrize("n", N_GRID)
@pytest.mark.parametrize("kind", ["mi", "mi_nz"])
def test_discrete_layout_built_on_the_device_from_csc(kind, n, p, top):
    m = discrete_csc(n, p, top)
    nnz_of = np.diff(m.indptr)
    last = 64 * ((n - 1) // 64)
    assert nnz_of[1] == 0 and nnz_of[2] == n and m.indices[m.indptr[3]] == last  # empty, full, only the last plane word
    assert set(r for r in (0, 63, 64, n - 1) if r < n) <= set(m.indices[m.indptr[0]:m.indptr[1]].tolist())
    assert top <= 2 or (m.indices[-1] == n - 1 and m.data[-1] == top and (m.data == top).sum() == 1)
    exp = discrete_reference(kind, n, p, top)
    assert exp["levels"][1] == 1 and exp["levels"][2] == min(top, 2) and max(exp["max_vals"]) == top
    for index in INDEX_DTYPES:
        got = engine_state(kind, csc_tensor(m, index), max_k=max_k_of(top))
        assert got.keys() == exp.keys()
        for key in exp:
            assert got[key] == exp[key], (index, key)
    if n == 130 and p == 129 and not (kind == "mi_nz" and top == 61):
        # the comparison is not one of empty lists.  (mi_nz at 62 levels is: its tests size every variable at L - 1 = 61 levels,
        # tests.jl:200-203, and 130 samples over 60 x 60 cells are below hps = 5 per cell -- no pair has power, on either path)
        assert len(exp["l0"][1]) > 0 and len(exp["edges"]) > 0


@pytest.mark.parametrize("values", [np.int64, np.float64, np.uint8], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("top", [2, 3], ids=["plane_form", "generic_form"])
@pytest.mark.parametrize("n,p", [(65, 5), (130, 129)])
@pytest.mark.parametrize("kind", ["mi", "mi_nz"])
def test_level_values_of_another_dtype_are_cast_on_the_device_before_the_library_reads_them(kind, n, p, top, values):
    """values() that are not Int32 already (Int64 is torch's default for integers): Engine.set_data casts them on the device, on torch's
    current stream, and the library reads them on a stream of its own -- also when the current stream is not the default one, which
    nothing but the helper's own synchronisation orders before the library's kernels"""
    m = discrete_csc(n, p, top)
    exp = discrete_reference(kind, n, p, top)
    side = torch.cuda.Stream(device=GPU)
    for stream in (torch.cuda.default_stream(GPU), side):
        with torch.cuda.stream(stream):
            t = csc_tensor(m, values=m.data.astype(values))
            assert t.values().dtype == torch.from_numpy(np.zeros(1, values)).dtype
            got = engine_state(kind, t, max_k=2)
        assert got == exp, stream


def test_level_values_that_a_cast_would_change_are_refused_before_any_library_call():
    m = discrete_csc(65, 5, 2)
    eng = fw.Engine("mi", 65, 5, max_k=2)
    for bad, match in ((1.5, "non-integral"), (float("nan"), "non-integral"), (-1.0, "0 .. 2\\^31 - 1"), (2.0**31, "0 .. 2\\^31 - 1")):
        v = m.data.astype(np.float64)
        v[3] = bad
        with pytest.raises(ValueError, match=match):
            eng.set_data(csc_tensor(m, values=v))
    with pytest.raises(ValueError, match="0 .. 2\\^31 - 1"):
        eng.set_data(csc_tensor(m, values=np.where(np.arange(m.nnz) == 3, 2**31, m.data.astype(np.int64))))
    eng.close()


# ---- layout build, fz_nz: dense-resident and CSC-resident -------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True], ids=["dense_resident", "csc_resident"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("p", P_GRID)
@pytest.mark.parametrize("n", N_GRID)
def test_fz_nz_layouts_built_on_the_device_from_csc(n, p, dtype, resident):
    m = fznz_csc(n, p, dtype)
    assert m.data.dtype == dtype and (np.float32(m.data) == 0).sum() == 3  # a stored 0.0, a -0.0, a value that rounds to 0.0f
    triple = (m.indptr, m.indices, m.data)  # (as stored: scipy's constructor would not drop them, as_csc would -- both are absences)
    exp = engine_state("fz_nz", _Triple(triple, m.shape), csc_resident=resident)
    for index in INDEX_DTYPES:
        got = engine_state("fz_nz", csc_tensor(m, index), csc_resident=resident)
        assert got.keys() == exp.keys()
        for key in exp:
            assert got[key] == exp[key], (index, key)
    if n == 130 and p == 129:
        assert len(exp["l0"][1]) > 0 and len(exp["edges"]) > 0


class _Triple(tuple):
    """a (colptr, rowval, nzval) tuple as Engine.set_data takes it, with the shape engine_state reads"""

    def __new__(cls, triple, shape):
        t = super().__new__(cls, triple)
        t.shape = shape
        return t


# ---- refusals: the host form's code, the column's number, and the context stays usable --------------------------------------------
def swapped_rows(m, col):
    """the arrays of m with the first two rows of column `col` swapped"""
    bad = m.copy()
    a = bad.indptr[col]
    assert bad.indptr[col + 1] - a >= 2
    bad.indices[[a, a + 1]] = bad.indices[[a + 1, a]]
    return bad


def row_equal_n(m, col):
    bad = m.copy()
    bad.indices[bad.indptr[col + 1] - 1] = m.shape[0]
    return bad


def with_value(m, col, value):
    bad = m.copy()
    bad.data[bad.indptr[col]] = value
    return bad


def host_triple(m, dtype):
    return (m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(dtype))


def answers(eng, exp):
    """the engine still answers for the table it held: the level-0 lists and a batch of tests, to the bit"""
    l0 = eng.pw_univar_neighbors()
    assert (l0["off"].tolist(), l0["idx"].tolist(), bits(l0["stat"]).tolist(), bits(l0["pval"]).tolist()) == exp["l0"]
    assert result_bits(eng.test_batch(*jobs(eng.p))) == exp["tests"]


@pytest.mark.parametrize("kind", ["mi", "mi_nz"])
def test_a_defective_level_triple_is_refused_as_the_host_refuses_it(kind):
    n, p, col = 65, 5, 3
    good = discrete_csc(n, p, 2)
    exp_state = discrete_reference(kind, n, p, 2)
    cases = [(swapped_rows(good, 0), -1, 0), (row_equal_n(good, col), -1, col), (with_value(good, col, 0), -5, col), (with_value(good, col, 62), -5, col)]
    for bad, code, column in cases:
        host, dev = fw.Engine(kind, n, p, max_k=2, n_obs_min=10), fw.Engine(kind, n, p, max_k=2, n_obs_min=10)
        dev.set_data(csc_tensor(good))
        exp = refusal(lambda: host.set_data(host_triple(bad, np.int32)))  # (the tuple form: the arrays as they are, nothing canonicalised)
        assert exp is not None and exp[0] == code and "column %d" % column in exp[1]
        for index in INDEX_DTYPES:
            assert refusal(lambda: dev.set_data(csc_tensor(bad, index))) == exp, index
            answers(dev, exp_state)  # a refused triple left the context as it was
        host.close(), dev.close()


@pytest.mark.parametrize("resident", [False, True], ids=["dense_resident", "csc_resident"])
def test_a_defective_fz_nz_triple_is_refused_as_the_host_refuses_it(resident):
    n, p, col = 65, 5, 3
    good = fznz_csc(n, p, np.float32)
    exp_state = engine_state("fz_nz", good, csc_resident=resident)
    for bad, column in ((swapped_rows(good, 0), 0), (row_equal_n(good, col), col)):
        host, dev = fw.Engine("fz_nz", n, p, max_k=2, n_obs_min=10), fw.Engine("fz_nz", n, p, max_k=2, n_obs_min=10)
        dev.set_data(csc_tensor(good), csc_resident=resident)
        exp = refusal(lambda: host.set_data(host_triple(bad, np.float32), csc_resident=resident))
        assert exp is not None and exp[0] == -1 and "column %d" % column in exp[1]
        got = refusal(lambda: dev.set_data(csc_tensor(bad), csc_resident=resident))
        # (the message begins with the entry point's name, which carries _dev here; the code and the rest are the host form's)
        assert got is not None and got[0] == exp[0] and got[1].replace("_dev:", ":") == exp[1]
        if resident:
            answers(dev, exp_state)  # the CSC-resident upload builds beside what the context holds: it is as it was
        else:  # the dense-resident upload scatters in place: no data until the next good upload, as in the host form
            no_data = refusal(lambda: dev.pw_univar_neighbors()), refusal(lambda: host.pw_univar_neighbors())
            assert no_data[0] is not None and no_data[1] is not None and no_data[0][0] == no_data[1][0]
        dev.set_data(csc_tensor(good), csc_resident=resident)
        answers(dev, exp_state)
        host.close(), dev.close()


def test_recursive_pcor_off_on_the_resident_layout_stays_a_limit():
    m = fznz_csc(65, 5, np.float32)
    eng = fw.Engine("fz_nz", 65, 5, max_k=2, recursive_pcor=False)
    got = refusal(lambda: eng.set_data(csc_tensor(m), csc_resident=True))
    assert got is not None and got[0] == -5 and "recursive_pcor = 0" in got[1]
    eng.set_data(csc_tensor(m))
    eng.close()


def test_null_and_host_pointers_are_refused_without_a_dereference():
    L = fw.load_library()
    n, p = 65, 5
    m = discrete_csc(n, p, 2)
    mi, fz = fw.Engine("mi", n, p, max_k=2, n_obs_min=10), fw.Engine("fz_nz", n, p, max_k=2)
    h_cp, h_row, h_i, h_f = m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.int32), m.data.astype(np.float32)
    d_cp, d_row = torch.from_numpy(h_cp).to(GPU), torch.from_numpy(h_row).to(GPU)
    d_i, d_f, d_d = torch.from_numpy(h_i).to(GPU), torch.from_numpy(h_f).to(GPU), torch.from_numpy(m.data.astype(np.float64)).to(GPU)
    torch.cuda.synchronize()
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    dp = lambda t: ctypes.c_void_p(t.data_ptr())
    for entry, ctx, d_v, h_v in ((L.fw_set_data_csc_i32_dev, mi, d_i, h_i), (L.fw_set_data_csc_f32_dev, fz, d_f, h_f),
                                 (L.fw_set_data_csc_f32_resident_dev, fz, d_f, h_f)):
        good = [dp(d_cp), dp(d_row), dp(d_v)]
        for k, host_ptr in enumerate((hp(h_cp), hp(h_row), hp(h_v))):
            for bad_ptr, word in ((None, b"NULL"), (host_ptr, b"not device memory")):
                args = list(good)
                args[k] = bad_ptr
                assert entry(ctx.h, *args, m.nnz) == -1 and word in L.fw_last_error(ctx.h), (entry.__name__, k, word)
        assert entry(ctx.h, *good, m.nnz - 1) == -1 and b"colptr must run from 0 to nnz" in L.fw_last_error(ctx.h)  # (before any kernel)
        assert entry(ctx.h, *good, m.nnz) == 0
    rm, cm = np.zeros(n, np.uint8), np.zeros(p, np.uint8)
    no, po, nz = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
    o_cp, o_row = torch.empty(p + 1, dtype=torch.int64, device=GPU), torch.empty(m.nnz, dtype=torch.int32, device=GPU)
    o_i = torch.empty(m.nnz, dtype=torch.int32, device=GPU)
    tail = (hp(rm), hp(cm), ctypes.byref(no), ctypes.byref(po), ctypes.byref(nz), None)
    for front_end, d_v, h_v in ((L.fw_normalize_counts_csc_dev, d_i, h_i), (L.fw_normalize_abund_csc_dev, d_d, m.data.astype(np.float64))):
        good_in, good_out = [dp(d_cp), dp(d_row), dp(d_v)], [dp(o_cp), dp(o_row), dp(o_i)]
        for k, host_ptr in enumerate((hp(h_cp), hp(h_row), hp(h_v))):
            for bad_ptr in (None, host_ptr):
                args = list(good_in)
                args[k] = bad_ptr
                assert front_end(0, fw.FW_MI, n, p, *args, m.nnz, *good_out, None, *tail) == -1, (front_end.__name__, k)
        assert b"not device memory" in L.fw_last_error(None)
        for k, host_buf in enumerate((h_cp, h_row, h_i)):
            for bad_ptr in (None, hp(host_buf)):
                outs = list(good_out)
                outs[k] = bad_ptr
                assert front_end(0, fw.FW_MI, n, p, *good_in, m.nnz, *outs, None, *tail) == -1, (front_end.__name__, "out", k)
        assert b"output buffer is not device memory" in L.fw_last_error(None)
        assert front_end(0, fw.FW_MI, n, p, *good_in, m.nnz + 1, *good_out, None, *tail) == -1 and b"colptr must run from 0 to nnz" in L.fw_last_error(None)
        assert front_end(0, fw.FW_MI, n, p, *good_in, m.nnz, *good_out, None, *tail) == 0 and no.value > 0 and po.value > 0
    assert [a.tolist() for a in mi.levels()] == [discrete_reference("mi", n, p, 2)[k] for k in ("levels", "max_vals")]
    mi.close(), fz.close()


# ---- front-end -----------------------------------------------------------------------------------------------------------------
def same_front_end(got, exp, kind):
    """(data, row_mask, col_mask) of the tensor call against the scipy call: colptr, rowval, the values' bits and both masks; the dense
    output's bits for "fz" """
    assert all(isinstance(mask, np.ndarray) and mask.dtype == bool and np.array_equal(mask, e) for mask, e in zip(got[1:], exp[1:]))
    assert not exp[1].all() and not exp[2].all()  # both masks hold a False
    data = got[0]
    assert isinstance(data, torch.Tensor) and data.is_cuda and tuple(data.shape) == exp[0].shape
    if kind == "fz":
        assert isinstance(exp[0], np.ndarray) and data.layout == torch.strided and data.stride() == (1, data.shape[0])
        assert np.array_equal(bits(data.cpu().numpy()), bits(exp[0]))
        return
    assert sp.issparse(exp[0]) and data.layout == torch.sparse_csc
    values = data.values().cpu().numpy()
    assert values.dtype == exp[0].data.dtype
    assert np.array_equal(data.ccol_indices().cpu().numpy(), exp[0].indptr) and np.array_equal(data.row_indices().cpu().numpy(), exp[0].indices)
    assert np.array_equal(bits(values) if values.dtype.kind == "f" else values, bits(exp[0].data) if values.dtype.kind == "f" else exp[0].data)


FRONT_END = ([dict(test_name=t) for t in ("fz", "fz_nz", "mi", "mi_nz")] + [dict(test_name="fz", norm="tss"), dict(test_name="mi_nz", norm="tss-nonzero-binned"),
             dict(test_name="mi_nz", n_bins=5, rank_method="dense")])


@pytest.mark.parametrize("kw", FRONT_END, ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_front_end_on_a_sparse_csc_device_tensor(kw):
    m = count_csc()
    assert m.shape == (200, 40)
    kw = dict(kw)
    test_name = kw.pop("test_name")
    exp = fw.normalize_counts(m, test_name, **kw)
    kind = "fz" if (test_name == "fz" and "norm" not in kw) else "sparse"
    for index in INDEX_DTYPES:
        same_front_end(fw.normalize_counts(csc_tensor(m, index), test_name, **kw), exp, kind)
    same_front_end(fw.normalize_counts(csc_tensor(m, values=m.data.astype(np.float64)), test_name, **kw), exp, kind)  # (integral floats are counts)


@pytest.mark.parametrize("kw", [dict(test_name=t) for t in ("fz", "fz_nz", "mi", "mi_nz")] + [dict(test_name="fz", norm="tss")],
                         ids=lambda kw: "-".join(str(v) for v in kw.values()))
def test_front_end_on_a_real_valued_sparse_csc_device_tensor(kw):
    m = count_csc().astype(np.float64) * 0.5
    kw = dict(kw)
    test_name = kw.pop("test_name")
    exp = fw.normalize_abundances(m, test_name, **kw)
    kind = "fz" if (test_name == "fz" and "norm" not in kw) else "sparse"
    for index in INDEX_DTYPES:
        same_front_end(fw.normalize_abundances(csc_tensor(m, index), test_name, **kw), exp, kind)


def test_front_end_value_checks_run_on_the_stored_values():
    m = count_csc()
    with pytest.raises(TypeError, match="integer counts"):
        fw.normalize_counts(csc_tensor(m, values=m.data * 0.5), "mi_nz")
    with pytest.raises(ValueError, match=r"\[0, 2\^31 - 1\]"):
        fw.normalize_counts(csc_tensor(m, values=m.data.astype(np.int64) - 10 ** 6), "mi_nz")
    with pytest.raises(ValueError, match="a negative value"):
        fw.normalize_abundances(csc_tensor(m, values=m.data - 1.0e6), "fz")
    with pytest.raises(ValueError, match="outside"):
        fw.normalize_abundances(csc_tensor(m, values=m.data * 2.0 ** 100), "fz", norm="tss")
    # a stored zero in a count table: the host form's code, the column's number (here through the tuple form, which keeps it stored)
    bad = with_value(m, 7, 0)
    exp = refusal(lambda: _counts_csc_host(bad))
    got = refusal(lambda: fw.normalize_counts(csc_tensor(bad), "mi_nz"))
    assert exp is not None and exp[0] == -1 and "column 7" in exp[1] and "stored zero" in exp[1]
    assert got is not None and got[0] == exp[0] and got[1].replace("_dev:", ":") == exp[1]
    for broken in (swapped_rows(m, 7), row_equal_n(m, 7)):
        exp, got = refusal(lambda: _counts_csc_host(broken)), refusal(lambda: fw.normalize_counts(csc_tensor(broken), "mi_nz"))
        assert exp is not None and exp[0] == -1 and "column 7" in exp[1]
        assert got is not None and got[0] == exp[0] and got[1].replace("_dev:", ":") == exp[1]


def _counts_csc_host(m):
    """fw_normalize_counts_csc on the arrays of m as they are (engine.CSC: as_csc hands it on untouched)"""
    from flashweave_jl_amd.engine import CSC
    return fw.normalize_counts(CSC(m.indptr.astype(np.int64), m.indices.astype(np.int32), m.data.astype(np.int32), tuple(m.shape)), "mi_nz")


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def same_network(got, exp):
    assert edge_bits(got["edges"]) == edge_bits(exp["edges"]) and len(exp["edges"]) > 0
    assert got["variable_ids"] == exp["variable_ids"] and got["meta_variable_mask"] == exp["meta_variable_mask"]
    assert got["rejections"] == exp["rejections"]
    assert got["counters"]["table_on_device"] is True and got["parameters"]["table_on_device"] is True and got["counters"]["sparse_input"] is True
    assert "table_on_device" not in exp["counters"] and "table_on_device" not in exp["parameters"] and exp["counters"]["sparse_input"] is True
    assert {k: v for k, v in got["parameters"].items() if k != "table_on_device"} == exp["parameters"]
    assert set(got["counters"]) - set(exp["counters"]) == {"table_on_device"}
    assert got["counters"]["data_resident_bytes"] == exp["counters"]["data_resident_bytes"]


def mode(test_name):
    return dict(sensitive=test_name.startswith("fz"), heterogeneous=test_name.endswith("_nz"), max_k=2)


@pytest.mark.parametrize("test_name", ["mi", "mi_nz", "fz_nz", "fz", "fz_nz-csc_resident", "fz-track_rejections"])
def test_learn_network_on_a_sparse_csc_device_tensor(test_name):
    m = count_csc()
    test_name, _, option = test_name.partition("-")
    kw = dict(mode(test_name), **({option: True} if option else {}))
    exp, got = fw.learn_network(m, **kw), fw.learn_network(csc_tensor(m), **kw)
    same_network(got, exp)
    assert got["counters"]["normalized_on_device"] and got["counters"]["csc_resident"] is (option == "csc_resident")
    assert option != "track_rejections" or len(exp["rejections"]) > 0


@pytest.mark.parametrize("test_name", ["mi", "mi_nz", "fz_nz"])
def test_normalize_data_then_learn_network_stays_on_the_device(test_name):
    m = count_csc()
    r = fw.normalize_data(csc_tensor(m), test_name=test_name)
    e = fw.normalize_data(m, test_name=test_name)
    assert r["data"].is_cuda and r["data"].layout == torch.sparse_csc and r["header"] == e["header"]
    assert np.array_equal(r["row_mask"], e["row_mask"]) and np.array_equal(r["meta_mask"], e["meta_mask"])
    got = fw.learn_network(r["data"], normalize=False, header=r["header"], **mode(test_name))
    exp = fw.learn_network(e["data"], normalize=False, header=e["header"], **mode(test_name))
    same_network(got, exp)
    assert edge_bits(got["edges"]) == edge_bits(fw.learn_network(m, **mode(test_name))["edges"])


def test_real_valued_tensor_end_to_end():
    m = count_csc().astype(np.float64) * 0.5
    kw = dict(mode("fz_nz"), abundances=True)
    same_network(fw.learn_network(csc_tensor(m), **kw), fw.learn_network(m, **kw))


# ---- what a sparse device tensor is not served with -----------------------------------------------------------------------------
def test_every_refusal_names_its_option_and_the_way_out(monkeypatch):
    m = count_csc()
    t = csc_tensor(m)
    coo, r = torch.from_numpy(m.toarray()).to(GPU).to_sparse(), m.tocsr()
    csr = torch.sparse_csr_tensor(torch.from_numpy(r.indptr).to(GPU), torch.from_numpy(r.indices).to(GPU), torch.from_numpy(r.data).to(GPU), size=r.shape)
    assert coo.layout == torch.sparse_coo and csr.layout == torch.sparse_csr
    called = []
    monkeypatch.setattr(fw.api, "normalize_counts", lambda *a, **k: called.append("normalize_counts"))
    monkeypatch.setattr(fw.api, "normalize_abundances", lambda *a, **k: called.append("normalize_abundances"))
    monkeypatch.setattr(fw.api, "Engine", lambda *a, **k: called.append("Engine"))
    both = [(dict(meta_data=np.arange(200.0).reshape(200, 1)), "meta_data"), (dict(meta_mask=np.arange(40) == 0), "meta_mask"),
            (dict(extra_data=[(m, None)]), "extra_data"), (dict(prec=64), "prec=64"), (dict(device_normalize=False), "device_normalize=False")]
    for entry in (fw.learn_network, fw.normalize_data):
        for kw, name in both:
            with pytest.raises(ValueError, match=r"%s with a table in GPU memory.*tensor\.cpu\(\)" % name):
                entry(t, **kw)
        with pytest.raises(ValueError, match=r"abundances=True.*tensor\.cpu\(\)"):
            entry(csc_tensor(m, values=m.data * 0.5))
        with pytest.raises(ValueError, match=r"device=1 .*tensor\.cpu\(\)"):
            entry(t, device=1)
        for other in (coo, csr):  # every other sparse layout: the old refusal
            with pytest.raises(ValueError, match=r"sparse torch tensor.*tensor\.cpu\(\)"):
                entry(other)
    with pytest.raises(ValueError, match=r"distributed=True with a table in GPU memory.*tensor\.cpu\(\)"):
        fw.learn_network(t, distributed=True)
    with pytest.raises(ValueError, match=r"sparse data with sensitive=True, heterogeneous=False, normalize=False"):
        fw.learn_network(t, normalize=False)
    with pytest.raises(ValueError, match=r"csc_resident=True is served for sensitive=True, heterogeneous=True"):
        fw.learn_network(t, sensitive=False, heterogeneous=True, csc_resident=True)
    assert called == []  # before any library call
    eng = fw.Engine("fz", 200, 40, prec=64)
    with pytest.raises(ValueError, match="prec=64"):
        eng.set_data(t)
    eng.close()
    eng = fw.Engine("fz", 200, 40)
    with pytest.raises(ValueError, match="dense matrix"):
        eng.set_data(t)
    eng.close()
    eng = fw.Engine("mi", 200, 40)
    with pytest.raises(ValueError, match="csc_resident=True"):
        eng.set_data(t, csc_resident=True)
    with pytest.raises(ValueError, match="sparse torch tensor"):
        eng.set_data(coo)
    not_canonical = torch.sparse_csc_tensor(t.ccol_indices().flip(0), t.row_indices(), t.values(), size=t.shape)
    with pytest.raises(ValueError, match="not canonical"):  # (column pointers that step down: refused with torch ops, nothing is launched)
        eng.set_data(not_canonical)
    eng.close()
