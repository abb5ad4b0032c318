"""The sparse-CSC device-tensor interface as far as a host without a GPU sees it: the five *_dev entry points for CSC triples are
declared and exported, the ABI number did not move, and the refusals of learn_network / normalize_data -- which all come before any
library call -- keep their order and wording, read with a stand-in for a tensor in GPU memory (tests/csc_device_tables.py).  What needs
a real tensor lives in tests/test_gpu_csc_device_tables.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import flashweave_jl_amd as fw
from tests.csc_device_tables import FakeSparseCscTensor, count_csc
from tests.util import ROOT

CSC_DEV_SYMBOLS = ("fw_set_data_csc_i32_dev", "fw_set_data_csc_f32_dev", "fw_set_data_csc_f32_resident_dev", "fw_normalize_counts_csc_dev",
                   "fw_normalize_abund_csc_dev")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fw.lib_path()):
        fw.build_library()
    return fw.load_library()


def test_the_five_entry_points_are_in_the_header_and_declared(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flashweave_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(fw.lib_path())
    for name in CSC_DEV_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes, name  # load_library declared it
    # the arguments of the host forms plus nnz (and, for the front-ends, opts passed directly)
    assert len(lib.fw_set_data_csc_i32_dev.argtypes) == len(lib.fw_set_data_csc_i32.argtypes) + 1
    assert len(lib.fw_set_data_csc_f32_resident_dev.argtypes) == len(lib.fw_set_data_csc_f32_resident.argtypes) + 1
    assert len(lib.fw_normalize_counts_csc_dev.argtypes) == len(lib.fw_normalize_counts_csc_opts.argtypes) + 1
    assert len(lib.fw_normalize_abund_csc_dev.argtypes) == len(lib.fw_normalize_abund_csc_opts.argtypes) + 1


def test_the_abi_number_did_not_move(lib):
    assert lib.fw_abi_version() == 6
    assert "#define FW_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "flashweave_amd.h")).read()


def test_a_cpu_sparse_csc_tensor_is_not_a_device_table():
    m = count_csc()
    t = torch.sparse_csc_tensor(torch.from_numpy(m.indptr), torch.from_numpy(m.indices), torch.from_numpy(m.data), size=m.shape)
    assert fw.engine.is_sparse_csc_tensor(t) and not fw.engine.is_device_tensor("x", t)
    assert not fw.engine.is_sparse_csc_tensor(m) and not fw.engine.is_sparse_csc_tensor(np.zeros((2, 2)))
    assert not fw.engine.is_sparse_csc_tensor(torch.zeros(2, 2)) and not fw.engine.is_sparse_csc_tensor(torch.zeros(2, 2).to_sparse())


def test_csc_resident_with_a_cpu_sparse_csc_tensor_keeps_the_refusal_of_a_table_that_is_not_sparse():
    m = count_csc()
    t = torch.sparse_csc_tensor(torch.from_numpy(m.indptr), torch.from_numpy(m.indices), torch.from_numpy(m.data), size=m.shape)
    with pytest.raises(ValueError, match=r"csc_resident=True needs sparse data \(a scipy\.sparse matrix\)"):
        fw.api._resolve_mode("fz_nz", 32, t, True, True, True)
    assert fw.api._resolve_mode("fz_nz", 32, m, True, True, True) == (True, True, True)


@pytest.fixture
def stand_in(monkeypatch):
    """learn_network / normalize_data take a FakeSparseCscTensor for a tensor in GPU memory; every library call is recorded"""
    called = []
    for mod in (fw.api, fw.engine):
        monkeypatch.setattr(mod, "is_device_tensor", lambda who, d: isinstance(d, FakeSparseCscTensor))
        monkeypatch.setattr(mod, "is_sparse_csc_tensor", lambda d: isinstance(d, FakeSparseCscTensor) and d.layout == torch.sparse_csc)
    monkeypatch.setattr(fw.api, "normalize_counts", lambda *a, **k: called.append("normalize_counts"))
    monkeypatch.setattr(fw.api, "normalize_abundances", lambda *a, **k: called.append("normalize_abundances"))
    monkeypatch.setattr(fw.api, "Engine", lambda *a, **k: called.append("Engine"))
    return called


def test_the_refusals_of_a_sparse_csc_device_tensor_their_order_and_wording(stand_in):
    m = count_csc()
    t = FakeSparseCscTensor(m, torch.sparse_csc)
    # the options in the order they are refused: each call holds every later one as well, and names the first
    order = [("meta_data", np.arange(200.0).reshape(200, 1), "meta_data"), ("meta_mask", np.arange(40) == 0, "meta_mask"),
             ("extra_data", [(m, None)], "extra_data"), ("prec", 64, "prec=64"), ("device_normalize", False, "device_normalize=False")]
    for entry in (fw.learn_network, fw.normalize_data):
        for k in range(len(order)):
            kw = {name: value for name, value, _ in order[k:]}
            with pytest.raises(ValueError, match=r"^%s: %s with a table in GPU memory is not supported: .*; pass tensor\.cpu\(\) instead$"
                               % (entry.__name__, order[k][2])):
                entry(t, **kw)
        with pytest.raises(ValueError, match=r"device=1 while the tensor lives on cuda:0.*tensor\.cpu\(\)"):
            entry(t, device=1)
        with pytest.raises(ValueError, match=r"does not hold integral counts.*abundances=True.*tensor\.cpu\(\)"):
            entry(FakeSparseCscTensor(m * 0.5, torch.sparse_csc))
        with pytest.raises(ValueError, match=r"2-D samples x variables table of a numeric dtype.*tensor\.cpu\(\)"):
            entry(FakeSparseCscTensor(m, torch.sparse_csc, dtype=torch.complex64))
    with pytest.raises(ValueError, match=r"^learn_network: distributed=True with a table in GPU memory is not supported"):
        fw.learn_network(t, distributed=True, device=1)  # (before the device mismatch)
    with pytest.raises(ValueError, match=r"device=1 while"):
        fw.learn_network(t, device=1, normalize=False, csc_resident=True)  # (csc_resident=True itself is no refusal for this layout)
    # the sparse refusal and the mode's own, after those of the tensor
    with pytest.raises(ValueError, match=r"sparse data with sensitive=True, heterogeneous=False, normalize=False is not supported"):
        fw.learn_network(t, normalize=False)
    with pytest.raises(ValueError, match=r"csc_resident=True is served for sensitive=True, heterogeneous=True \(fz_nz\) only"):
        fw.learn_network(t, csc_resident=True)
    with pytest.raises(ValueError, match=r"csc_resident=True with recursive_pcor=False is not supported"):
        fw.learn_network(t, heterogeneous=True, csc_resident=True, recursive_pcor=False)
    with pytest.raises(ValueError, match=r"abundances=True with normalize=False"):
        fw.learn_network(t, abundances=True, normalize=False)
    assert stand_in == []  # every one of them before any library call


@pytest.mark.parametrize("layout", [torch.sparse_coo, torch.sparse_csr, torch.sparse_bsr, torch.sparse_bsc])
def test_every_other_sparse_layout_keeps_the_old_refusal(stand_in, layout):
    t = FakeSparseCscTensor(count_csc(), layout)
    for entry in (fw.learn_network, fw.normalize_data):
        with pytest.raises(ValueError, match=r"sparse torch tensor.*tensor\.cpu\(\)"):  # (what tests/test_gpu_device_tables.py matches)
            entry(t)
        with pytest.raises(ValueError, match=r"a sparse torch tensor is not supported: scipy\.sparse is the sparse interface.*to_sparse_csc\(\)"):
            entry(t, meta_mask=np.arange(40) == 0)  # (the layout is looked at first)
    assert stand_in == []


def test_a_served_call_reaches_the_front_end_and_the_engine_with_the_tensor_itself(stand_in, monkeypatch):
    """no host copy on the way: what normalize_counts and Engine.set_data receive is the caller's object / the front-end's output"""
    t = FakeSparseCscTensor(count_csc(), torch.sparse_csc)
    seen = {}

    class Out:
        shape = (199, 39)

    def front_end(c, name, **kw):
        seen["front_end"] = (c, name)
        return Out, np.ones(200, bool), np.ones(40, bool)

    class Eng:
        L = None

        def __init__(self, *a, **k):
            pass

        def set_data(self, mat, csc_resident=False):
            seen["set_data"] = (mat, csc_resident)

        def lgl(self, **kw):
            return dict(edges={}, rejections={})

        def counters(self):
            return {}

        def close(self):
            pass

        def data_resident_bytes(self):
            return 0

    monkeypatch.setattr(fw.api, "normalize_counts", front_end)
    monkeypatch.setattr(fw.api, "Engine", Eng)
    r = fw.learn_network(t, heterogeneous=True, csc_resident=True)
    assert seen["front_end"] == (t, "fz_nz") and seen["set_data"] == (Out, True)
    assert r["counters"]["sparse_input"] is True and r["counters"]["table_on_device"] is True and r["parameters"]["table_on_device"] is True
    assert r["counters"]["csc_resident"] is True and r["counters"]["normalized_on_device"] is True
    seen.clear()
    r = fw.learn_network(t, sensitive=False, normalize=False)
    assert "front_end" not in seen and seen["set_data"] == (t, False) and r["counters"]["sparse_input"] is True
