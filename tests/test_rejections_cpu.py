"""CPU checks of the rejection log (learn_network(track_rejections=True)).

The checker of the GPU tests (tests/test_gpu_rejections.py) is tests/hiton_rej_ref.py: the restated driver with the rejection branch
of update_sig_result! (hiton.jl:71-76).  Here it is anchored -- tracking changes no network, every record is a real non-significant
test of the oracle over variables the target could hold, and accepted + rejected = the univariate neighbours -- and the inputs are
shown to cover both phases, every set size, tests without power and stops far beyond a job's first window, so that the GPU comparison
cannot pass vacuously.  Also: the file format of save_rejections / load_rejections (io.jl:248-318) and the fw_rejection ABI."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import flashweave_jl_amd as fw
from flashweave_jl_amd import io as fio
from tests import hiton_exact_ref as H
from tests import hiton_rej_ref as HR
from tests.util import ROOT

KINDS = ["fz", "fz_nz", "mi", "mi_nz"]
ALPHA = 0.01


@pytest.fixture(scope="module")
def oracles():
    return HR.make_oracles()


@pytest.fixture(scope="module")
def oracles300():
    return HR.make_oracles(p=300, n=600)


@pytest.fixture(scope="module")
def nets(oracles):
    """(kind, max_k, fast_elim) -> tracked network on rounds of 16 targets"""
    out = {}
    for kind in KINDS:
        orc, disc, _ = oracles[kind]
        for max_k in (3, 5):
            for fast_elim in (True, False):
                out[(kind, max_k, fast_elim)] = HR.learn(orc, disc, max_k=max_k, feed_forward=True, round_size=16, fast_elim=fast_elim)
    return out


def _records(net):
    return [(T, c, r) for T, d in net["rejections"].items() for c, r in d.items()]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ff,R", [(True, 1), (True, 16), (False, 0)])
@pytest.mark.parametrize("fast_elim,no_red_tests", [(True, True), (False, True), (False, False)])
def test_tracking_changes_no_network(oracles, kind, ff, R, fast_elim, no_red_tests):
    orc, disc, _ = oracles[kind]
    kw = dict(max_k=3, feed_forward=ff, round_size=R, fast_elim=fast_elim, no_red_tests=no_red_tests)
    a, b = HR.learn(orc, disc, **kw), H.learn(orc, disc, **kw)
    for key in ("pc_off", "pc_idx", "pc_weight", "pc_pval"):
        assert a[key].tobytes() == b[key].tobytes(), key
    assert a["edges"] == b["edges"] and a["n_cond_tests"] == b["n_cond_tests"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("max_k", [3, 5])
@pytest.mark.parametrize("fast_elim", [True, False])
def test_records_are_the_oracles_tests(oracles, nets, kind, max_k, fast_elim):
    orc, disc, _ = oracles[kind]
    net = nets[(kind, max_k, fast_elim)]
    n_obs_min = orc.auto_n_obs_min(-1, 5, max_k)
    nb = orc.level0(alpha=ALPHA, hps=5, n_obs_min=n_obs_min, FDR=True)
    for T, c, r in _records(net):
        assert not (r["pval"] < ALPHA and r["suff_power"])
        assert len(r["pool"]) > 0 and set(r["Zs"]) <= set(r["pool"]) and len(r["Zs"]) <= max_k
        assert T not in r["pool"] and c not in r["pool"]
        o, e = int(nb["off"][T]), int(nb["off"][T + 1])
        assert set(r["pool"]) <= set(int(v) for v in nb["idx"][o:e])  # what T could hold: its univariate neighbours
        if r["num_tests"] == 0:  # tests.jl:293-296: no test at all
            assert r["Zs"] == () and r["frac"] == 0.0 and (r["stat"], r["pval"], r["df"], r["suff_power"]) == (0.0, 1.0, 0, False)
            continue
        if kind == "fz_nz":  # (its tests run on the row view of (T, c): Oracle.test_subsets over exactly Zs restates that)
            t = orc.test_subsets(T, c, list(r["Zs"]), max_k=len(r["Zs"]), alpha=ALPHA, hps=5, n_obs_min=n_obs_min)
        else:
            t = orc.test(T, c, list(r["Zs"]), hps=5, n_obs_min=n_obs_min)
        got = (t["stat"], t["pval"], t["df"], bool(t["suff_power"])) if isinstance(t, dict) else tuple(t)
        assert got == (r["stat"], r["pval"], r["df"], r["suff_power"]), (T, c, r, got)
    # accepted + rejected = the alpha-significant univariate neighbours, disjointly, for every target that ran HITON-PC
    levels = orc.levels()[0] if disc else None
    for T in range(orc.p):
        o, e = int(nb["off"][T]), int(nb["off"][T + 1])
        uni = {int(nb["idx"][i]) for i in range(o, e) if nb["pval"][i] < ALPHA}
        pc = set(int(v) for v in net["pc_idx"][net["pc_off"][T]:net["pc_off"][T + 1]])
        rej = set(net["rejections"].get(T, {}))
        if levels is not None and levels[T] < 2:
            assert not pc and not rej
            continue
        assert not (pc & rej) and (pc | rej) == uni, T


def test_inputs_cover_the_cases(nets):
    for kind in KINDS:
        for max_k in (3, 5):
            recs = _records(nets[(kind, max_k, True)])
            n_i = sum(1 for _, _, r in recs if r["phase"] == 0)
            assert n_i > 0 and len(recs) - n_i > 0, (kind, max_k, n_i, len(recs))  # both phases
            if kind != "mi_nz":
                assert {len(r["Zs"]) for _, _, r in recs if r["num_tests"] > 0} >= set(range(1, max_k + 1)), (kind, max_k)
        assert sum(1 for _, _, r in _records(nets[(kind, 3, False)]) if r["phase"] == 1) > 0
    assert sum(1 for _, _, r in _records(nets[("mi", 5, True)]) if not r["suff_power"]) > 0
    assert sum(1 for _, _, r in _records(nets[("mi_nz", 3, True)]) if not r["suff_power"]) > 0


def test_p300_stops_cross_the_first_window(oracles300):
    # first windows: 16 ranks (discrete kinds), 256 (fz) -- what the reference gives on this table, no more is claimed
    orc, disc, _ = oracles300["mi"]
    for fast_elim in (True, False):
        net = HR.learn(orc, disc, max_k=3, feed_forward=True, round_size=16, fast_elim=fast_elim)
        assert max(r["num_tests"] for _, _, r in _records(net)) > 16
    orc, disc, _ = oracles300["fz"]
    net = HR.learn(orc, disc, max_k=3, feed_forward=True, round_size=16, fast_elim=False)
    assert max(r["num_tests"] for _, _, r in _records(net)) > 256


def _as_api(rej):
    return {T: {c: (r["Zs"], (r["stat"], r["pval"], r["df"], r["suff_power"]), (r["num_tests"], r["frac"])) for c, r in d.items()}
            for T, d in rej.items()}


@pytest.mark.parametrize("kind", ["fz", "fz_nz", "mi_nz"])
def test_save_load_rejections_round_trip(nets, kind, tmp_path):
    rej = _as_api(nets[(kind, 3, True)]["rejections"])
    path = str(tmp_path / "rej.tsv")
    fio.save_rejections(path, rej, digits=5)
    lines = open(path).read().split("\n")
    assert lines[0] == "Edge\tRejecting_set\tStat\tP_value\tNum_tests\tPerc_tested\tDf\tSuffPower"
    T0 = min(rej)
    c0 = min(rej[T0])
    first = lines[1].split("\t")
    assert first[0] == "%d <-> %d" % (T0 + 1, c0 + 1)  # 1-based ids in the file
    assert first[1] == ",".join(str(z + 1) for z in rej[T0][c0][0]) and first[7] in ("true", "false")
    back = fio.load_rejections(path)
    assert {T: set(d) for T, d in back.items()} == {T: set(d) for T, d in rej.items()}
    for T, d in rej.items():
        for c, (zs, (stat, pval, df, pw), (nt, frac)) in d.items():
            bzs, (bstat, bpval, bdf, bpw), (bnt, bfrac) = back[T][c]
            assert (bzs, bdf, bpw, bnt) == (zs, df, pw, nt)  # integers exact
            for x, y in ((stat, bstat), (pval, bpval), (frac, bfrac)):  # floats to the rounding (test/io.jl:9 compare_rejections)
                assert y == round(x, 5)
    # the result object of learn_network is accepted as well
    fio.save_rejections(path, {"rejections": rej})
    assert fio.load_rejections(path) == back


def test_empty_log_file(tmp_path):
    path = str(tmp_path / "none.tsv")
    fio.save_rejections(path, {})
    assert open(path).read() == "# No rejections found, you may have forgotten to specify 'track_rejections' when running FlashWeave"
    assert fio.load_rejections(path) == {}


def test_fw_rejection_layout_and_symbols(tmp_path):
    from flashweave_jl_amd import engine as E
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "flashweave_amd.h"', 'int main(void) {',
           'printf("sizeof %zu\\n", sizeof(fw_rejection));']
    for f, _ in E._Rejection._fields_:
        src.append('printf("%s %%zu\\n", offsetof(fw_rejection, %s));' % (f, f))
    src.append('return 0; }')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(cfile)], check=True)
    hdr = dict((ln.split()[0], int(ln.split()[1])) for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert hdr["sizeof"] == ctypes.sizeof(E._Rejection) == E.REJECTION_DTYPE.itemsize == 88
    for f, _ in E._Rejection._fields_:
        assert getattr(E._Rejection, f).offset == hdr[f] == E.REJECTION_DTYPE.fields[f][1], f
    # no padding: the fields fill the struct
    assert sum(ctypes.sizeof(t) for _, t in E._Rejection._fields_) == 88
    if not os.path.exists(fw.lib_path()):
        fw.build_library()
    raw = ctypes.CDLL(fw.lib_path())
    for name in ("fw_set_track_rejections", "fw_rejections_count", "fw_rejections_get"):
        assert hasattr(raw, name), name
    assert fw.load_library().fw_abi_version() == 6


def test_learn_network_takes_the_keyword():
    import inspect
    sig = inspect.signature(fw.learn_network)
    assert sig.parameters["track_rejections"].default is False
    assert inspect.signature(fw.Engine.lgl).parameters["track_rejections"].default is False
