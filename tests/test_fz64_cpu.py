"""CPU tests of the Float64 Fisher-z mode (learn_network(prec=64)): the ABI additions, the shared Float64 pcor_rec header
(csrc/fw_pcor64.h, compiled natively through tests/native/pcor64_check.cpp) against the oracle's Float64 path, and the argument
rules of learn_network / Engine that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flashweave_jl_amd as fw
from flashweave_jl_amd import engine as E
from oracle import oracle as O
from tests.util import ROOT, load_norm


def test_library_exports_the_f64_entry_points():
    L = C.CDLL(E.lib_path())
    for name in ("fw_set_data_dense_f64", "fw_set_cor_mat_f64", "fw_get_cor_mat_f64"):
        assert hasattr(L, name), name
    L.fw_abi_version.restype = C.c_int
    assert L.fw_abi_version() == 6  # new entry points only: no struct changed


def _cases(p, rng, m):
    X, Y, Zs = [], [], []
    for _ in range(m):
        k = int(rng.integers(0, 6))
        v = rng.choice(p, size=k + 2, replace=False)
        X.append(int(v[0])); Y.append(int(v[1])); Zs.append(tuple(int(t) for t in v[2:]))
    # duplicated conditioning variables and Z == X (the cases tests/test_gpu_fz.py::test_single_tests_bit_exact adds)
    X += [1, 2, 3, 4]; Y += [5, 6, 7, 8]; Zs += [(9, 9), (11, 12, 11), (3, 8), (10, 4, 10, 12, 4)]
    return X, Y, Zs


def test_pcor64_header_is_bit_identical_to_the_oracle(tmp_path):
    clr = load_norm("clr_adapt", np.float64)
    cm = np.asfortranarray(O.cor(clr, "f64"))
    assert cm.dtype == np.float64
    p = cm.shape[0]
    orc = O.Oracle("fz", cor_mat=cm, n_obs=clr.shape[0])
    X, Y, Zs = _cases(p, np.random.default_rng(3), 4000)
    rec = np.zeros((len(X), 8), np.int32)
    for t, (x, y, z) in enumerate(zip(X, Y, Zs)):
        rec[t, :3] = (x, y, len(z))
        rec[t, 3:3 + len(z)] = z
    exe, fin, fout = str(tmp_path / "pcor64_check"), str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "native", "pcor64_check.cpp")], check=True)
    with open(fin, "wb") as f:
        f.write(np.array([p, len(X)], np.int32).tobytes())
        f.write(cm.tobytes(order="F"))
        f.write(rec.tobytes())
    r = subprocess.run([exe, fin, fout], check=True, capture_output=True, text=True)
    assert r.stdout.strip() == "ok %d" % len(X)
    got = np.fromfile(fout, dtype=np.float64)
    exp = np.array([orc.test(x, y, z, n_obs_min=0)[0] for x, y, z in zip(X, Y, Zs)])
    assert got.view(np.uint64).tolist() == exp.view(np.uint64).tolist()
    sizes = {len(z) for z in Zs}
    assert sizes == {0, 1, 2, 3, 4, 5}


def _counts():
    return np.random.default_rng(0).integers(0, 50, size=(40, 12))


def test_learn_network_refuses_other_precisions():
    for prec in (16, 128, 0):
        with pytest.raises(ValueError, match="prec"):
            fw.learn_network(_counts(), prec=prec)


def test_learn_network_refuses_f64_without_the_matrix_path():
    with pytest.raises(ValueError, match="prec=64 with recursive_pcor=False"):
        fw.learn_network(_counts(), prec=64, recursive_pcor=False)
    with pytest.raises(ValueError, match="prec=64 with dense_cor=False"):
        fw.learn_network(_counts(), prec=64, dense_cor=False)


def test_engine_prec_keyword_rules():
    with pytest.raises(ValueError, match="prec"):
        fw.Engine("fz", 40, 12, prec=16)
    for kind in ("fz_nz", "mi", "mi_nz"):
        with pytest.raises(ValueError, match="prec=64"):
            fw.Engine(kind, 40, 12, prec=64)
