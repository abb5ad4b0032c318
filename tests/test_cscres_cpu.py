"""CSC-resident fz_nz layout, the parts that need no device: the position arithmetic of csrc/fw_cscres.h (native check, plain and
under the host sanitizers), the two ABI additions, and the refusals of learn_network(csc_resident=True) / Engine.set_data, which all
happen before any device call."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "cscres_check.cpp")
INC = os.path.join(ROOT, "flashweave.jl_amd", "csrc")


def _compile(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", INC, "-o", exe, SRC], check=True)
    return exe


def test_position_function_finds_every_entry(tmp_path):
    # n = 1, 63, 64, 65, 128, 130 and 16 448; fills 0, 3 %, 50 % and 100 %; an empty column, a full column, columns whose only
    # entry is row n-1 / row 0, an empty last column, a table without any entry (tests/native/cscres_check.cpp)
    r = subprocess.run([_compile(tmp_path, "cscres_check", [])], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr


def test_position_function_under_host_sanitizers(tmp_path):
    # host code only.  The flags must compile, link and start a trivial program here; otherwise the leg is skipped with the reason
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    pexe = str(tmp_path / "probe")
    flags = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    c = subprocess.run(["g++", "-std=c++17", *flags, "-o", pexe, str(probe)], capture_output=True, text=True)
    if c.returncode != 0:
        pytest.skip("g++ does not accept -fsanitize=address,undefined here: " + c.stderr.strip()[-300:])
    r = subprocess.run([pexe], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("a -fsanitize=address,undefined program does not start here: " + r.stderr.strip()[-300:])
    r = subprocess.run([_compile(tmp_path, "cscres_check_san", flags)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), r.stdout + r.stderr[-3000:]


def test_new_symbols_exported_bound_and_abi_unchanged():
    if not os.path.exists(fw.lib_path()):
        fw.build_library()
    lib = fw.load_library()
    raw = ctypes.CDLL(fw.lib_path())
    assert hasattr(raw, "fw_set_data_csc_f32_resident") and hasattr(raw, "fw_data_resident_bytes")
    assert lib.fw_abi_version() == 6  # new functions only: no struct or existing signature changed
    hdr = open(os.path.join(ROOT, "include", "flashweave_amd.h")).read()
    assert "int fw_set_data_csc_f32_resident(" in hdr and "int fw_data_resident_bytes(" in hdr
    assert lib.fw_set_data_csc_f32_resident.argtypes == [ctypes.c_void_p] * 4
    assert lib.fw_data_resident_bytes.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int64)]
    # NULL context: refused before anything touches a device
    assert lib.fw_set_data_csc_f32_resident(None, None, None, None) == -1
    assert lib.fw_data_resident_bytes(None, None) == -1


def _table():
    rng = np.random.default_rng(3)
    return rng.integers(0, 6, size=(40, 12)) * (rng.random((40, 12)) < 0.4)


@pytest.mark.parametrize("data, kwargs, words", [
    # dense data
    (_table(), dict(sensitive=True, heterogeneous=True), "sparse"),
    # every other mode
    (sp.csc_matrix(_table()), dict(sensitive=True, heterogeneous=False), "fz_nz"),
    (sp.csc_matrix(_table()), dict(sensitive=False, heterogeneous=True), "fz_nz"),
    (sp.csc_matrix(_table()), dict(sensitive=False, heterogeneous=False), "fz_nz"),
    # streamed conditional tests
    (sp.csc_matrix(_table()), dict(sensitive=True, heterogeneous=True, recursive_pcor=False), "recursive_pcor"),
])
def test_learn_network_refuses_by_name_before_any_device_call(data, kwargs, words, monkeypatch):
    # (on the parent commit the keyword itself is unknown: TypeError)
    def no_device(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    monkeypatch.setattr(fw.api, "Engine", no_device)
    monkeypatch.setattr(fw.api, "normalize_counts", no_device)
    with pytest.raises(ValueError) as ei:
        fw.learn_network(data, csc_resident=True, **kwargs)
    assert "csc_resident" in str(ei.value) and words in str(ei.value)


def test_engine_set_data_refuses_by_name():
    # Engine.__new__: the checks come before the context is touched, so no device is needed to see them
    m = sp.csc_matrix(_table().astype(np.float32))
    for name, data, words in (("fz_nz", _table().astype(np.float32), "dense"), ("mi_nz", m, "fz_nz"), ("fz", m, "fz_nz")):
        eng = fw.Engine.__new__(fw.Engine)
        eng.test_name, eng.n, eng.p, eng.prec, eng.h = name, 40, 12, 32, None
        with pytest.raises(ValueError) as ei:
            eng.set_data(data, csc_resident=True)
        assert "csc_resident" in str(ei.value) and words in str(ei.value)


def test_a_build_without_the_entry_points_is_refused_by_name():
    # an older library (loaded for A/B profiling) lacks the two functions: a named refusal, not an AttributeError
    m = sp.csc_matrix(_table().astype(np.float32))
    eng = fw.Engine.__new__(fw.Engine)
    eng.test_name, eng.n, eng.p, eng.prec, eng.h, eng.L = "fz_nz", 40, 12, 32, None, object()
    with pytest.raises(fw.FlashWeaveError) as ei:
        eng.set_data(m, csc_resident=True)
    assert ei.value.code == -5 and "csc_resident" in str(ei.value) and "fw_set_data_csc_f32_resident" in str(ei.value)
    with pytest.raises(fw.FlashWeaveError) as ei:
        eng.data_resident_bytes()
    assert "fw_data_resident_bytes" in str(ei.value)
