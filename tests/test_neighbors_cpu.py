"""learn_neighbors / Engine.neighbors without a device: the interface, every refusal before an engine exists, the resolution of
targets as a pure function, and -- on the oracle alone -- that the tables of tests/test_gpu_neighbors.py hold the variables its
comparisons need (a comparison of empty rows would be vacuous)."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import api
from oracle import oracle as O
from tests import api_trace
from tests import neighbors_tables as NT


def test_the_interface_exists():
    """The test that fails without the feature."""
    sig = inspect.signature(fw.learn_neighbors).parameters
    assert list(sig)[:3] == ["data", "targets", "meta_data_path"]
    for gone in ("feed_forward", "round_size", "distributed"):
        assert gone not in sig
    theirs = inspect.signature(fw.learn_network).parameters
    assert set(theirs) - set(sig) == {"feed_forward", "round_size", "distributed"} and set(sig) - set(theirs) == {"targets"}
    for k in set(sig) & set(theirs):  # the same defaults, the same kinds
        assert sig[k].default == theirs[k].default and sig[k].kind == theirs[k].kind, k
    nb = inspect.signature(fw.Engine.neighbors).parameters
    assert list(nb) == ["self", "targets", "round_size", "edge_dict", "fast_elim", "no_red_tests", "track_rejections"]
    assert (nb["round_size"].default, nb["edge_dict"].default, nb["fast_elim"].default, nb["no_red_tests"].default,
            nb["track_rejections"].default) == (0, True, True, True, False)


@pytest.fixture
def nothing_runs(monkeypatch):
    """Engine and the two device front-ends replaced by recorders -> the list of what was called"""
    called = []
    monkeypatch.setattr(fw.api, "normalize_counts", lambda *a, **k: called.append("normalize_counts"))
    monkeypatch.setattr(fw.api, "normalize_abundances", lambda *a, **k: called.append("normalize_abundances"))
    monkeypatch.setattr(fw.api, "Engine", lambda *a, **k: called.append("Engine"))
    return called


def test_the_form_of_targets_is_refused_before_anything_runs(nothing_runs):
    counts = api_trace.counts()
    for bad, what in (([], "empty"), ((), "empty"), (["X1", 2], "mixed"), ([0, "X2"], "mixed"), ([True], "not a list of names or indices"),
                      ([1.0], "not a list of names or indices"), ("X1", "must be a list"), (3, "must be a list"), (None, "must be a list"),
                      (np.zeros((2, 2), int), "must be a list")):
        with pytest.raises(ValueError, match=r"learn_neighbors: targets.*%s" % what):
            fw.learn_neighbors(counts, bad)
    for kw in (dict(feed_forward=False), dict(round_size=0), dict(distributed=False), dict(verbose=True)):
        with pytest.raises(TypeError, match=r"learn_neighbors: unsupported options \['%s'\]" % list(kw)[0]):
            fw.learn_neighbors(counts, ["X1"], **kw)
    with pytest.raises(TypeError):  # options are keywords, as for learn_network
        fw.learn_neighbors(counts, ["X1"], None, True)
    assert nothing_runs == []


def test_learn_networks_refusals_under_this_name(nothing_runs):
    counts, csc = api_trace.counts(), sp.csc_matrix(api_trace.counts())
    het = dict(sensitive=True, heterogeneous=True)
    for data, kw, msg in ((counts, dict(prec=16), "prec=16 is not supported"),
                          (counts, dict(meta_data_path="meta.tsv"), "meta_data_path goes with a data path"),
                          (counts, dict(transposed=True), "transposed=True is served for the path form"),
                          (csc, dict(device_normalize=False), "sparse data with device_normalize=False"),
                          (csc, dict(prec=64), "sparse data with prec=64"),
                          (counts, dict(csc_resident=True, **het), "csc_resident=True needs sparse data"),
                          (csc, dict(csc_resident=True, sensitive=False), "csc_resident=True is served for"),
                          (counts, dict(prec=64, recursive_pcor=False), "prec=64 with recursive_pcor=False"),
                          (counts, dict(abundances=True, normalize=False), "abundances=True with normalize=False"),
                          (counts, dict(meta_mask=np.ones(8, bool)), "meta_mask marks every column"),
                          (counts, dict(extra_data=[(counts[:-1], None)]), r"extra_data\[0\] has 5 rows"),
                          (api_trace.prepared("fz"), dict(normalize=False, meta_data=api_trace.META), "meta_data with normalize=False")):
        with pytest.raises(ValueError, match="learn_neighbors: " + msg):
            fw.learn_neighbors(data, ["X1"], **kw)
    assert nothing_runs == []


def test_targets_are_resolved_before_an_engine_exists(nothing_runs):
    """What needs the final variable_ids is refused behind the (host) front-end and before Engine is constructed."""
    counts = api_trace.counts().copy()
    counts[:, 3] = 0  # normalisation drops an empty column
    host = dict(device_normalize=False, sensitive=True, heterogeneous=True)
    with pytest.raises(ValueError, match=r"learn_neighbors: targets holds the column index 8, which is out of range for the 8 columns"):
        fw.learn_neighbors(counts, [0, 8], **host)
    with pytest.raises(ValueError, match=r"learn_neighbors: targets holds the column index -1"):
        fw.learn_neighbors(counts, [-1], **host)
    with pytest.raises(ValueError, match=r"learn_neighbors: targets names 'otu9', which matches no variable"):
        fw.learn_neighbors(counts, ["otu1", "otu9"], header=api_trace.HEADER, **host)
    with pytest.raises(ValueError, match=r"learn_neighbors: targets names 'otu3', which is not among the variables normalisation kept"):
        fw.learn_neighbors(counts, ["otu1", "otu3"], header=api_trace.HEADER, **host)
    with pytest.raises(ValueError, match=r"learn_neighbors: targets names 'X4', which is not among the variables normalisation kept"):
        fw.learn_neighbors(counts, [1, 3], **host)
    with pytest.raises(ValueError, match=r"learn_neighbors: targets lists the variable 'X2' twice"):
        fw.learn_neighbors(counts, [1, 4, 1], **host)
    with pytest.raises(ValueError, match=r"learn_neighbors: targets names 'a', which matches 2 columns \(0, 2\)"):
        fw.learn_neighbors(counts, ["a"], header=["a", "b", "a", "c", "d", "e", "f", "g"], **host)
    assert nothing_runs == []


# ---- resolution as a pure function ----
def _names(targets, cols, header):
    return api._targets_names("f", targets, cols, header)


def test_names_and_integers():
    ids = ["a", "b", "c", "d"]
    assert api.resolve_targets("f", ["c", "a"], ids) == [2, 0]  # the caller's order
    assert api.resolve_targets("f", _names([2, 0], 4, ids), ids) == [2, 0]
    assert api.resolve_targets("f", _names([np.int64(3)], 4, ids), ids) == [3]
    assert api._targets_form("f", np.array([1, 2])) == "columns" and api._targets_form("f", ("a",)) == "names"
    with pytest.raises(ValueError, match="f: targets.*empty"):
        api._targets_form("f", [])
    with pytest.raises(ValueError, match="f: targets.*mixed"):
        api._targets_form("f", ["a", 1])


def test_callers_header_and_default_header():
    assert _names([0, 2], 3, None) == ["X1", "X3"]
    assert _names([0, 2], 3, ["u", "v", "w"]) == ["u", "w"]
    assert _names(["w"], 3, ["u", "v", "w"]) == ["w"]  # a name is looked up in the final ids, whatever the header says
    with pytest.raises(ValueError, match="f: targets holds the column index 3, which is out of range for the 3 columns"):
        _names([3], 3, None)
    with pytest.raises(ValueError, match="f: targets holds the column index 2, which the header of 2 names does not name"):
        _names([2], 3, ["u", "v"])  # (learn_network lets a short header pass: zip truncates)


def test_meta_columns_move_last_and_extra_tables_first():
    # a table under meta_mask: columns 1 and 3 are meta variables and come last in variable_ids
    header = ["o0", "m1", "o2", "m3", "o4"]
    final = ["o0", "o2", "o4", "m1", "m3"]
    assert api.resolve_targets("f", _names([1, 2, 4], 5, header), final, header) == [3, 1, 2]
    assert api.resolve_targets("f", _names([0, 3], 5, None), ["X1", "X3", "X5", "X2", "X4"]) == [0, 4]
    # extra_data: [last extra, ..., first extra, data]; an integer is a column of the main table, a name may be an extra table's
    final = ["b0", "b1", "its0", "its1", "o0", "o2"]
    assert api.resolve_targets("f", _names([0, 2], 3, ["o0", "o1", "o2"]), final, ["o0", "o1", "o2", "its0", "its1", "b0", "b1"]) == [4, 5]
    assert api.resolve_targets("f", ["its1", "o0", "b0"], final) == [3, 4, 0]


def test_dropped_columns_and_duplicates():
    given, final = ["a", "b", "c", "d", "e"], ["b", "c", "e"]
    assert api.resolve_targets("f", _names([2, 4], 5, given), final, given) == [1, 2]  # two columns dropped in front of 'e'
    with pytest.raises(ValueError, match=r"f: targets names 'a', 'd', which are not among the variables normalisation kept"):
        api.resolve_targets("f", ["a", "c", "d", "a"], final, given)
    with pytest.raises(ValueError, match=r"f: targets names 'z', which matches no variable"):
        api.resolve_targets("f", ["a", "z"], final, given)  # (an unknown name first: nothing was dropped under it)
    with pytest.raises(ValueError, match=r"f: targets names 'c', which matches 2 columns \(1, 3\)"):
        api.resolve_targets("f", ["c"], ["b", "c", "e", "c"], given)
    with pytest.raises(ValueError, match=r"f: targets lists the variable 'c' twice"):
        api.resolve_targets("f", ["b", "c", "c"], final, given)
    with pytest.raises(ValueError, match=r"f: targets lists the variable 'X2' twice"):
        api.resolve_targets("f", _names([1, 0, 1], 3, None), ["X1", "X2", "X3"])


def test_learn_neighbors_composes_the_shared_stages(monkeypatch):
    """The calls a learn_neighbors run makes, on the recording engine of tests/api_trace.py: learn_network's, with neighbors(ids) in
    the place of lgl, and the result's extra keys."""
    log = api_trace._LOG
    del log[:]

    class Rec(api_trace.RecordingEngine):
        def neighbors(self, targets, **kw):
            log.append(["neighbors", list(targets), dict(kw)])
            return dict(edges={(1, 4): 0.5}, rejections={}, pc_off=np.array([0, 0, 2, 2, 2, 3, 3, 3]), pc_idx=np.array([4, 0, 1], np.int32),
                        pc_weight=np.array([0.5, -0.25, 0.5]), pc_pval=np.array([1e-3, 2e-3, 1e-3]))
    monkeypatch.setattr(fw.api, "Engine", Rec)
    counts = api_trace.counts().copy()
    counts[:, 0] = 0  # dropped in front of the targets: column 5 is variable 4
    r = fw.learn_neighbors(counts, [5, 2], sensitive=True, heterogeneous=True, device_normalize=False, fast_elim=False, max_k=2)
    assert r["variable_ids"] == ["X%d" % j for j in range(2, 9)] and r["targets"] == [4, 1]
    assert r["neighbors"] == {4: {1: (0.5, 1e-3)}, 1: {4: (0.5, 1e-3), 0: (-0.25, 2e-3)}} and list(r["neighbors"][1]) == [4, 0]  # PC order
    assert r["parameters"]["targets"] == 2 and r["parameters"]["schedule"] == "targets (no feed-forward: each neighbourhood on its own)"
    assert r["parameters"]["feed_forward"] is False and r["parameters"]["distributed"] == 0 and r["parameters"]["max_k"] == 2
    names = [c[0] for c in log]
    assert names == ["Engine", "set_data", "neighbors", "counters", "data_resident_bytes", "close"]
    assert log[2][1:] == [[4, 1], dict(edge_dict=True, fast_elim=False, no_red_tests=True, track_rejections=False)]
    assert set(r) == {"edges", "variable_ids", "meta_variable_mask", "parameters", "counters", "rejections", "targets", "neighbors"}


# ---- the GPU tests' tables, on the oracle alone ----
def oracle_of(kind, data):
    if kind == "fz":
        return O.Oracle("fz", cor_mat=O.cor(data.astype(np.float64), "f32"), n_obs=data.shape[0])
    if kind == "fz_nz":
        return O.Oracle("fz_nz", data=data.astype(np.float64))
    return O.Oracle(kind, data, sparse=True, max_k=3)


@pytest.mark.parametrize("p", sorted(NT.SIZES))
@pytest.mark.parametrize("kind", NT.KINDS)
def test_the_gpu_tables_hold_what_the_comparisons_need(kind, p):
    data = NT.table(kind, p)
    assert data.shape[1] == p
    orc = oracle_of(kind, data)
    l0 = orc.level0(alpha=0.01, n_obs_min=20 if kind in ("fz", "fz_nz") else orc.auto_n_obs_min(-1, 5, 3))
    exp = orc.learn(max_k=3, feed_forward=False)
    tg = NT.choose_targets(l0["off"], l0["idx"])
    deg, kept = np.diff(l0["off"]), np.diff(exp["pc_off"])
    assert len(tg["single"]) == 1 and deg[tg["single"][0]] == 1
    assert len(tg["none"]) == 1 and deg[tg["none"][0]] == 0
    assert len(tg["pair"]) == 2 and tg["pair"][1] in l0["idx"][l0["off"][tg["pair"][0]]:l0["off"][tg["pair"][0] + 1]]
    top = tg["longest"][0]
    assert deg[top] == deg.max() >= 4
    assert kept[top] < deg[top] and kept[top] > 0  # a conditional test removes a level-0 neighbour of a listed target, and some stay
    assert exp["n_cond_tests"] > 0
    orc.close()
