"""bench.py's option surface and its --dump-outputs writer (no GPU: the writer is fed a network of the Engine.lgl shape)."""
import os

import numpy as np
import pytest

import bench


def _net(rng, n_edges, p, n_dir):
    return {"edge_src": rng.integers(0, p, n_edges).astype(np.int32), "edge_dst": rng.integers(0, p, n_edges).astype(np.int32),
            "edge_weight": rng.standard_normal(n_edges), "pc_off": np.sort(rng.integers(0, n_dir, p + 1)).astype(np.int64),
            "pc_idx": rng.integers(0, p, n_dir).astype(np.int32), "pc_weight": rng.standard_normal(n_dir),
            "pc_pval": rng.random(n_dir)}


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_exact_float64(tmp_path):
    net = _net(np.random.default_rng(1), 500, 300, 2000)
    bench.dump_outputs(net, str(tmp_path / "d"))
    assert sorted(os.listdir(tmp_path / "d")) == sorted(k + ".npy" for k in bench.DUMP_KEYS)
    for k in bench.DUMP_KEYS:
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == np.float64
        if k == "pc_tested":
            np.testing.assert_array_equal(got, np.ones(2000))
        else:
            np.testing.assert_array_equal(got, net[k].astype(np.float64))


def test_dump_outputs_untested_entries_are_finite_and_marked(tmp_path):
    # whitelist-admitted neighbours carry (NaN, NaN) in the directed lists (fw_hiton.cpp advance(), hiton.jl:20-30)
    net = _net(np.random.default_rng(3), 50, 40, 300)
    untested = np.zeros(300, bool)
    untested[::7] = True
    net["pc_weight"][untested] = np.nan
    net["pc_pval"][untested] = np.nan
    bench.dump_outputs(net, str(tmp_path / "d"))
    for k in bench.DUMP_KEYS:
        assert np.isfinite(np.load(tmp_path / "d" / (k + ".npy"))).all(), k
    np.testing.assert_array_equal(np.load(tmp_path / "d" / "pc_tested.npy"), (~untested).astype(np.float64))
    for k in ("pc_weight", "pc_pval"):
        got = np.load(tmp_path / "d" / (k + ".npy"))
        np.testing.assert_array_equal(got[~untested], net[k][~untested])
        assert (got[untested] == 0.0).all()


def test_dump_outputs_refuses_other_non_finite_values(tmp_path):
    net = _net(np.random.default_rng(4), 50, 40, 300)
    net["edge_weight"][3] = np.inf
    with pytest.raises(SystemExit, match="edge_weight"):
        bench.dump_outputs(net, str(tmp_path / "d"))


def test_dump_outputs_sampled_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200_000)
    net = _net(np.random.default_rng(2), 100, 50, 40_000)
    for d in ("a", "b"):
        bench.dump_outputs(net, str(tmp_path / d))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 200_000
    big = np.load(tmp_path / "a" / "pc_pval.npy")
    assert 0 < big.size < net["pc_pval"].size
    assert np.isin(big, net["pc_pval"]).all()  # entries of the array, not made-up values
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "edge_weight.npy"), net["edge_weight"])  # small arrays whole
    for k in bench.DUMP_KEYS:  # the sample is fixed: two dumps of the same network are the same files
        np.testing.assert_array_equal(np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy")))
