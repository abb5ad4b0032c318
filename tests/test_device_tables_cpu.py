"""The device-resident table interface as far as a host without a GPU sees it: the four *_dev entry points are declared and exported,
the ABI number did not move, a CPU torch.Tensor keeps going through np.asarray, and a tensor of a device type that has no bytes is
refused by name.  What needs a tensor in GPU memory lives in tests/test_gpu_device_tables.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import flashweave_jl_amd as fw
from tests.norm_mode_tables import bits, edge_table
from tests.util import ROOT

DEV_SYMBOLS = ("fw_set_data_dense_i32_dev", "fw_set_data_dense_f32_dev", "fw_normalize_counts_dev", "fw_normalize_abund_dev")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fw.lib_path()):
        fw.build_library()
    return fw.load_library()


def test_the_four_entry_points_are_in_the_header_and_declared(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "flashweave_amd.h")).read(), flags=re.S)
    raw = ctypes.CDLL(fw.lib_path())
    for name in DEV_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, hdr), name
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes, name  # load_library declared it
    assert len(lib.fw_normalize_counts_dev.argtypes) == len(lib.fw_normalize_counts_opts.argtypes)
    assert len(lib.fw_set_data_dense_i32_dev.argtypes) == 2


def test_the_abi_number_did_not_move(lib):
    assert lib.fw_abi_version() == 6
    assert "#define FW_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "flashweave_amd.h")).read()


@pytest.mark.parametrize("test_name", ["fz", "mi_nz"])
def test_a_cpu_tensor_is_an_array(test_name):
    """through np.asarray, as before: the host front-end gives what it gives for the numpy table"""
    x = edge_table()
    exp = fw.normalize_data(x, test_name=test_name, device_normalize=False)
    got = fw.normalize_data(torch.from_numpy(x), test_name=test_name, device_normalize=False)
    assert isinstance(got["data"], np.ndarray) and got["data"].dtype == exp["data"].dtype and got["data"].shape == exp["data"].shape
    assert np.array_equal(bits(got["data"]), bits(exp["data"]))
    assert got["header"] == exp["header"] and np.array_equal(got["row_mask"], exp["row_mask"])
    assert np.array_equal(got["meta_mask"], exp["meta_mask"])


def test_a_meta_tensor_is_refused_by_name():
    t = torch.empty((8, 4), dtype=torch.int32, device="meta")
    with pytest.raises(ValueError, match="'meta' device"):
        fw.normalize_data(t, test_name="mi")
    with pytest.raises(ValueError, match="'meta' device"):
        fw.learn_network(t)
    with pytest.raises(ValueError, match="'meta' device"):
        fw.normalize_counts(t, "mi")
    with pytest.raises(ValueError, match="'meta' device"):
        fw.normalize_abundances(t, "fz")
