"""Engine.neighbors / learn_neighbors / fw_learn_neighbors on the GPU: HITON-PC for chosen targets only.

What is compared with what:
  * a listed target's directed row with its row of the SAME engine's lgl(feed_forward=False), byte for byte (pc_idx order, pc_weight,
    pc_pval); unlisted rows are empty; the edges are make_symmetric_graph of the listed rows, recomputed here from the directed
    output (tests/neighbors_tables.py: symmetric_graph);
  * the full run itself with oracle.Oracle.learn(feed_forward=False), by the comparisons tests/test_gpu_fz.py, test_gpu_fznz.py and
    test_gpu_mi.py use for directed results: lists equal; fz / fz_nz weights equal; discrete weights to rtol 1e-11, atol 1e-15.
The tables are those of tests/neighbors_tables.py (p = 40 and 130); tests/test_neighbors_cpu.py checks on the oracle that they hold
a variable of every kind the target lists need and that conditional tests remove level-0 neighbours of listed targets.
The full run of a (kind, p) is computed once per module, under the default knobs, and never changed."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import io as fio
from flashweave_jl_amd import synth
from flashweave_jl_amd.engine import REJECTION_DTYPE, _LearnOpts
from oracle import oracle as O
from tests import neighbors_tables as NT

pytestmark = pytest.mark.gpu
KEYS = ("pc_idx", "pc_weight", "pc_pval")
LISTS = ("longest", "single", "none", "pair", "all")


def make_engine(kind, data, csc_resident=False, **kw):
    """an engine of `kind` that holds `data` (and, for fz with a matrix, its Pearson matrix)"""
    n, p = data.shape
    eng = fw.Engine(kind, n, p, **kw)
    if kw.get("prec") == 64:
        data = np.asarray(data, dtype=np.float64)
    eng.set_data(sp.csc_matrix(data) if csc_resident else data, csc_resident=csc_resident)
    if kind == "fz" and kw.get("dense_cor", True):
        eng.compute_cor()
    return eng


_CTX = {}


def ctx(kind, p):
    """(kind, p) -> the table, an engine that holds it, its full feed_forward=False run (with counters), level-0 lists and target lists:
    computed once, under the default knobs (a module fixture would run under the first test's monkeypatch as well)"""
    if (kind, p) not in _CTX:
        data = NT.table(kind, p)
        eng = make_engine(kind, data, max_k=3)
        l0 = eng.pw_univar_neighbors()
        eng.reset_counters()
        full = eng.lgl(feed_forward=False, round_size=0)
        _CTX[kind, p] = dict(kind=kind, p=p, data=data, eng=eng, full=full, counters=eng.counters(), l0=l0,
                             targets=NT.choose_targets(l0["off"], l0["idx"]))
    return _CTX[kind, p]


def check_rows(got, full, targets, p):
    """test 1: listed rows are the full run's bytes, unlisted rows are empty, the edges are the symmetric graph of the rows"""
    off, foff = got["pc_off"], full["pc_off"]
    assert off.shape == (p + 1,)
    listed = np.zeros(p, bool)
    listed[list(targets)] = True
    assert np.array_equal(np.diff(off), np.where(listed, np.diff(foff), 0))
    for t in targets:
        for key in KEYS:
            assert got[key][off[t]:off[t + 1]].tobytes() == full[key][foff[t]:foff[t + 1]].tobytes(), (t, key)
    assert got["edges"] == NT.symmetric_graph(off, got["pc_idx"], got["pc_weight"])
    if len(targets) == p:
        assert got["edges"] == full["edges"]
        for key in ("edge_src", "edge_dst", "edge_weight", "pc_off") + KEYS:
            assert got[key].tobytes() == full[key].tobytes(), key


# ---- 1. rows equal the full run ----
@pytest.mark.parametrize("p", sorted(NT.SIZES))
@pytest.mark.parametrize("kind", NT.KINDS)
def test_rows_equal_the_full_run(kind, p):
    c = ctx(kind, p)
    eng, full, tg = c["eng"], c["full"], c["targets"]
    assert all(len(tg[k]) > 0 for k in LISTS) and len(tg["pair"]) == 2
    deg, kept = np.diff(c["l0"]["off"]), np.diff(full["pc_off"])
    assert kept[tg["longest"][0]] < deg[tg["longest"][0]]  # a conditional test removed a level-0 neighbour of a listed target
    for which in LISTS:
        got = eng.neighbors(tg[which])
        check_rows(got, full, tg[which], p)
        if which == "none":
            assert len(got["pc_idx"]) == 0 and got["edges"] == {}
        if which == "pair":  # an edge between two listed targets is merged from both rows; in either order of the list
            a, b = tg["pair"]
            back = eng.neighbors([b, a])
            assert back["edges"] == got["edges"] and all(back[k].tobytes() == got[k].tobytes() for k in ("pc_off",) + KEYS)


@pytest.mark.parametrize("kind", NT.KINDS)
def test_the_full_run_equals_the_oracle(kind):
    """the reference of every comparison here against oracle.Oracle.learn(feed_forward=False), as the kinds' own test files compare"""
    c = ctx(kind, 130)
    data, full = c["data"], c["full"]
    if kind == "fz":
        orc = O.Oracle("fz", cor_mat=c["eng"].cor_mat(), n_obs=data.shape[0])
    elif kind == "fz_nz":
        orc = O.Oracle("fz_nz", data=data.astype(np.float64))
    else:
        orc = O.Oracle(kind, data, sparse=True, max_k=3)
    exp = orc.learn(max_k=3, feed_forward=False)
    assert np.array_equal(full["pc_off"], exp["pc_off"]) and np.array_equal(full["pc_idx"], exp["pc_idx"]) and len(exp["pc_idx"]) > 0
    if kind in ("fz", "fz_nz"):
        assert np.array_equal(full["pc_weight"], exp["pc_weight"], equal_nan=True)
        assert full["edges"] == exp["edges"]
    else:
        assert np.allclose(full["pc_weight"], exp["pc_weight"], rtol=1e-11, atol=1e-15, equal_nan=True)
        assert set(full["edges"]) == set(exp["edges"])
    assert c["counters"]["cond_tests_ref"] == exp["n_cond_tests"]
    orc.close()


# ---- 2. every path ----
SETTINGS = {"host_pool": (dict(FW_HOST_HITON="1"), 0),
            "device_from_one_target": (dict(FW_DEV_MIN_TARGETS="1"), 0),       # below every list: device schedule / rounds
            "device_from_three_targets": (dict(FW_DEV_MIN_TARGETS="3"), 0),    # above one and two targets, below all p
            "no_device": (dict(FW_DEV_MIN_TARGETS="1000"), 0),                 # above all p
            "no_light_targets": (dict(FW_DEV_MIN_TARGETS="1", FW_DH_LIGHT_DEG="0"), 0),
            "no_schedule": (dict(FW_DEV_MIN_TARGETS="1", FW_FZ_SCHED="0", FW_MI_SCHED="0"), 0),  # the device rounds of the round loop
            "round_size_1": (dict(FW_DEV_MIN_TARGETS="1"), 1),
            "round_size_7": (dict(FW_DEV_MIN_TARGETS="1"), 7),
            "round_size_1_default": ({}, 1),
            "round_size_7_default": ({}, 7)}
FZ_ON_THE_DEVICE = ("device_from_one_target", "device_from_three_targets", "no_light_targets", "no_schedule", "round_size_1", "round_size_7")


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("kind", ["fz", "mi"])
def test_every_path_gives_the_same_bits(kind, setting, monkeypatch):
    c = ctx(kind, 130)  # (the reference first: it is computed under the default knobs)
    env, round_size = SETTINGS[setting]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = make_engine(kind, c["data"], max_k=3)
    for which in LISTS:
        eng.reset_counters()
        got = eng.neighbors(c["targets"][which], round_size=round_size)
        check_rows(got, c["full"], c["targets"][which], 130)
        if which == "all":  # the counters count every job once, on whichever path it ran
            cn = eng.counters()
            assert (cn["cond_tests_ref"], cn["subsets_calls"]) == (c["counters"]["cond_tests_ref"], c["counters"]["subsets_calls"])
            # which path ran (only the job pool counts t_host_advance_s): a discrete list always takes the pool; 130 Fisher-z targets
            # take the device wherever the threshold lets a round of theirs
            assert (cn["t_host_advance_s"] > 0) == (kind == "mi" or setting not in FZ_ON_THE_DEVICE), cn
    eng.close()


# ---- 3. the modes of the host pool, each against its own full run ----
def _counts(p, n, seed, mode):
    return synth.generate(p, n, seed, mode=mode)


MODES = {"max_k_0_fz": ("fz", dict(max_k=0), {}),
         "max_k_0_mi": ("mi", dict(max_k=0), {}),
         "max_k_6_fz": ("fz", dict(max_k=6, max_tests=3000), {}),  # (the enumeration starts with the sets of six)
         "max_k_6_mi": ("mi", dict(max_k=6, max_tests=3000), {}),
         "prec_64": ("fz", dict(max_k=3, prec=64), {}),
         "no_recursive_pcor": ("fz", dict(max_k=3, recursive_pcor=False), {}),
         "no_recursive_pcor_no_matrix": ("fz", dict(max_k=3, recursive_pcor=False, dense_cor=False), {}),
         "five_levels": ("mi_nz", dict(max_k=3), {}),
         "csc_resident": ("fz_nz", dict(max_k=3, csc_resident=True), {}),
         "exact_elimination": ("fz", dict(max_k=3), dict(fast_elim=False, no_red_tests=True)),
         "exact_elimination_keeps_statistics": ("fz", dict(max_k=3), dict(fast_elim=False, no_red_tests=False)),
         "exact_elimination_mi": ("mi", dict(max_k=3), dict(fast_elim=False, no_red_tests=False))}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_modes_of_the_host_pool(mode):
    kind, eng_kw, run_kw = MODES[mode]
    if mode == "five_levels":  # what normalize_data(n_bins=5) gives: levels 0 .. 4, the generic discrete form
        data = np.ascontiguousarray(fw.normalize_data(_counts(130, NT.N_MI_NZ, 5, "F"), test_name="mi_nz", n_bins=5)["data"])
        assert data.max() == 4
    else:
        data = NT.table(kind, 40 if "max_k_6" in mode else 130)
    p = data.shape[1]
    eng = make_engine(kind, data, **eng_kw)
    l0 = eng.pw_univar_neighbors()
    tg = NT.choose_targets(l0["off"], l0["idx"])
    targets = [tg["longest"][0], tg["pair"][1]] + [v for v in range(p) if v not in (tg["longest"][0], tg["pair"][1])][-1:]
    assert len(set(targets)) == 3
    full = eng.lgl(feed_forward=False, round_size=0, **run_kw)
    got = eng.neighbors(targets, **run_kw)
    check_rows(got, full, targets, p)
    assert sum(len(got["pc_idx"][got["pc_off"][t]:got["pc_off"][t + 1]]) for t in targets) > 0
    if eng_kw["max_k"] == 0:  # the targets' level-0 rows
        for t in targets:
            assert np.array_equal(got["pc_idx"][got["pc_off"][t]:got["pc_off"][t + 1]], l0["idx"][l0["off"][t]:l0["off"][t + 1]])
    else:
        assert np.diff(full["pc_off"])[targets[0]] < np.diff(l0["off"])[targets[0]]  # conditional tests did run for a listed target
    eng.close()


# ---- 4. track_rejections ----
REJ_ENVS = {"default": {}, "device": dict(FW_DEV_MIN_TARGETS="1"), "host_pool": dict(FW_HOST_HITON="1")}


# (no "device" for the discrete kinds: a discrete list of targets always takes the job pool (choose_path), whose sums differ from the
# persistent kernel's in the last bits -- under that knob the full run and the list would run on two paths)
@pytest.mark.parametrize("kind,env", [(k, e) for k in NT.KINDS for e in sorted(REJ_ENVS) if not (e == "device" and k in ("mi", "mi_nz"))])
def test_the_rejection_log_is_the_full_runs_restricted(kind, env, monkeypatch):
    """The full run is this engine's, under the same knobs: FW_DEV_MIN_TARGETS=1 puts both runs of a Fisher-z kind on the device, where
    the records are written by the kernels."""
    env = REJ_ENVS[env]
    c = ctx(kind, 130)
    tg = c["targets"]
    targets = sorted(set(tg["pair"] + tg["single"] + tg["none"]))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = make_engine(kind, c["data"], max_k=3)
    whole = eng.lgl(feed_forward=False, round_size=0, track_rejections=True)
    rec = whole["rejection_records"]
    assert rec.dtype == REJECTION_DTYPE and len(rec) > 0
    got = eng.neighbors(targets, track_rejections=True)
    exp = rec[np.isin(rec["target"], targets)]
    assert len(exp) > 0 and got["rejection_records"].tobytes() == exp.tobytes()
    assert got["rejections"] == {t: v for t, v in whole["rejections"].items() if t in targets}
    plain = eng.neighbors(targets)
    assert plain["rejections"] == {} and plain["edges"] == got["edges"]
    for key in ("pc_off",) + KEYS + ("edge_src", "edge_dst", "edge_weight"):
        assert plain[key].tobytes() == got[key].tobytes(), key
    check_rows(got, whole, targets, 130)
    eng.close()


# ---- 5. additivity ----
@pytest.mark.parametrize("kind", NT.KINDS)
def test_counters_count_the_listed_targets_jobs_only(kind):
    c = ctx(kind, 130)
    eng, p = c["eng"], 130
    A, B = list(range(0, p, 2)), list(range(1, p, 2))
    total = {}
    for part in (A, B):
        eng.reset_counters()
        eng.neighbors(part, edge_dict=False)
        cn = eng.counters()
        for k in ("cond_tests_ref", "subsets_calls"):
            total[k] = total.get(k, 0) + cn[k]
    assert total == {k: c["counters"][k] for k in ("cond_tests_ref", "subsets_calls")} and total["cond_tests_ref"] > 0
    eng.reset_counters()
    eng.neighbors(c["targets"]["none"])
    cn = eng.counters()
    assert (cn["cond_tests_ref"], cn["subsets_calls"], cn["cond_tests_evaluated"], cn["subsets_launches"]) == (0, 0, 0, 0)


# ---- 6. one context, queried twice ----
@pytest.mark.parametrize("kind", NT.KINDS)
def test_one_context_queried_repeatedly(kind):
    c = ctx(kind, 40)
    data, p = c["data"], 40
    A, B = c["targets"]["pair"], [v for v in range(p) if v not in c["targets"]["pair"]][:5] + c["targets"]["single"]
    B = sorted(set(B))
    eng = make_engine(kind, data, max_k=3)
    eng.level0()
    eng.reset_counters()
    seq = [eng.neighbors(A), eng.neighbors(B), eng.lgl(feed_forward=False, round_size=0)]
    assert eng.counters()["level0_tests"] == 0  # level 0 ran once, before
    eng.close()
    for i, run in enumerate((lambda e: e.neighbors(A), lambda e: e.neighbors(B), lambda e: e.lgl(feed_forward=False, round_size=0))):
        fresh = make_engine(kind, data, max_k=3)
        exp = run(fresh)
        fresh.close()
        assert seq[i]["edges"] == exp["edges"]
        for key in ("pc_off",) + KEYS + ("edge_src", "edge_dst", "edge_weight"):
            assert seq[i][key].tobytes() == exp[key].tobytes(), (i, key)
    check_rows(seq[0], c["full"], A, p)
    check_rows(seq[1], c["full"], B, p)
    check_rows(seq[2], c["full"], list(range(p)), p)


# ---- 7. learn_neighbors end to end ----
def _raw(p=40, n=200, seed=5, mode="S"):
    return synth.generate(p, n, seed, mode=mode).astype(np.int64)


def _tensor(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda:0")


def _csc_tensor(x):
    import torch
    m = sp.csc_matrix(x)
    m.sort_indices()
    dev = "cuda:0"
    return torch.sparse_csc_tensor(torch.as_tensor(m.indptr.astype(np.int64), device=dev), torch.as_tensor(m.indices.astype(np.int64), device=dev),
                                   torch.as_tensor(m.data, device=dev), size=m.shape)


def _with_meta(sparse):
    x = _raw(seed=6).astype(np.float64)
    rows = np.arange(x.shape[0])
    x[:, 3], x[:, 17] = rows % 2, 0.5 + 0.25 * (rows % 7)
    mask = np.zeros(40, bool)
    mask[[3, 17]] = True
    header = [("meta%d" if m else "otu%d") % j for j, m in enumerate(mask)]
    return (sp.csc_matrix(x) if sparse else x), dict(meta_mask=mask, header=header)


def _path_case(tmp_path):
    path = str(tmp_path / "counts.tsv")
    fio.write_table(path, _raw(seed=7), ["otu%d" % j for j in range(40)])
    return path


def _dropped_column():
    x = _raw(seed=8)
    x[:, 2] = 0  # normalisation drops it: every later variable moves one place to the front
    return x


HET = dict(sensitive=True, heterogeneous=True)
# name -> (data, keywords, targets) with targets a function of the full result: the caller's list (names, or columns of data as passed)
E2E = {"numpy": (lambda tmp: _raw(), dict(sensitive=True), None),
       "numpy_mi": (lambda tmp: _raw(mode="F"), dict(sensitive=False), None),
       "scipy_meta_mask": (lambda tmp: _with_meta(True)[0], dict(HET, **_with_meta(True)[1]), lambda r: ["meta17", r["variable_ids"][0]]),
       "dense_tensor": (lambda tmp: _tensor(_raw()), dict(sensitive=True), None),
       "csc_tensor": (lambda tmp: _csc_tensor(_raw(seed=9)), HET, None),
       "extra_data": (lambda tmp: _raw(), dict(HET, extra_data=[(_raw(12, 200, 11), ["its%d" % j for j in range(12)])]),
                      lambda r: [next(h for h in r["variable_ids"] if h.startswith("its")), r["variable_ids"][-1]]),
       "path": (_path_case, HET, lambda r: ["otu5", "otu11"]),
       "columns_behind_a_dropped_one": (lambda tmp: _dropped_column(), dict(sensitive=True), lambda r: [11, 3, 39])}


@pytest.mark.parametrize("case", sorted(E2E))
def test_learn_neighbors_end_to_end(case, tmp_path):
    """learn_network(feed_forward=False) is the reference: learn_neighbors for every variable gives its edges entirely, and a list of
    targets gives the rows of that run and the symmetric graph of those rows alone."""
    make, kw, pick = E2E[case]
    data = make(tmp_path)
    full = fw.learn_network(data, feed_forward=False, **kw)
    ids = full["variable_ids"]
    every = fw.learn_neighbors(data, list(ids), **kw)
    assert every["variable_ids"] == ids and every["meta_variable_mask"] == full["meta_variable_mask"]
    assert every["edges"] == full["edges"] and len(full["edges"]) > 0 and every["targets"] == list(range(len(ids)))
    assert every["edges"] == _graph_of(every["neighbors"])
    busiest = max(every["neighbors"], key=lambda t: len(every["neighbors"][t]))
    targets = [ids[busiest], ids[(busiest + 7) % len(ids)]] if pick is None else pick(full)
    got = fw.learn_neighbors(data, targets, **kw)
    if case == "columns_behind_a_dropped_one":
        assert "X3" not in ids and got["targets"] == [ids.index("X%d" % (j + 1)) for j in targets] == [10, 2, 38]
    else:
        assert got["targets"] == [ids.index(t) for t in targets]
    assert list(got["neighbors"]) == got["targets"] and got["variable_ids"] == ids
    for t in got["targets"]:
        assert list(got["neighbors"][t].items()) == list(every["neighbors"][t].items()), t  # PC order, weight and p to the bit
    assert sum(len(v) for v in got["neighbors"].values()) > 0
    assert got["edges"] == _graph_of(got["neighbors"])
    assert got["parameters"]["targets"] == len(targets) and got["parameters"]["schedule"].startswith("targets (no feed-forward")
    assert got["parameters"]["feed_forward"] is False and got["rejections"] == {}
    if case == "path":  # save works unchanged
        got.save(str(tmp_path / "neighbourhoods.edgelist"))
        assert len(open(str(tmp_path / "neighbourhoods.edgelist")).read().strip().split("\n")) == 2 + len(got["edges"])


def _graph_of(neighbors):
    """{target: {neighbour: (weight, p)}} -> the symmetric graph of those rows (tests/neighbors_tables.py)"""
    p = 1 + max([t for t in neighbors] + [u for row in neighbors.values() for u in row])
    off, idx, w = [0], [], []
    for t in range(p):
        for u, (weight, _) in neighbors.get(t, {}).items():
            idx.append(u)
            w.append(weight)
        off.append(len(idx))
    return NT.symmetric_graph(off, idx, w)


def test_learn_neighbors_tracks_rejections(tmp_path):
    data = _raw()
    full = fw.learn_network(data, feed_forward=False, track_rejections=True)
    targets = sorted(full["rejections"])[:3]
    got = fw.learn_neighbors(data, targets, track_rejections=True)
    assert got["targets"] == targets and len(targets) == 3  # (integer targets, nothing dropped: columns are variables)
    assert got["rejections"] == {t: full["rejections"][t] for t in targets}
    got.save_rejections(str(tmp_path / "rejections.tsv"))


# ---- 8. the C-level refusals ----
def test_c_level_refusals_leave_the_context_usable():
    c = ctx("fz", 40)
    eng, L = make_engine("fz", c["data"], max_k=3), fw.load_library()
    ne = C.c_int64(0)

    def call(opts, targets, n=None, h=eng.h):
        t = None if targets is None else np.asarray(targets, dtype=np.int32)
        return L.fw_learn_neighbors(h, None if opts is None else C.byref(opts), None if t is None else t.ctypes.data_as(C.c_void_p),
                                    (0 if t is None else t.size) if n is None else n, C.byref(ne))
    ok = _LearnOpts(0, 0, 0, 1, 0, 0)
    for opts, targets, n, field in ((ok, None, 1, "targets is NULL"), (ok, [1], 0, "n_targets 0"), (ok, [1], -3, "n_targets -3"),
                                    (ok, [1, 40], None, r"targets[1] = 40"), (ok, [-1], None, r"targets[0] = -1"),
                                    (ok, [5, 2, 5], None, r"targets[2] = 5 is a duplicate"),
                                    (_LearnOpts(1, 0, 0, 1, 0, 0), [1], None, "feed_forward 1"),
                                    (_LearnOpts(0, 0, 0, 2, 0, 0), [1], None, "world_size 2"),
                                    (_LearnOpts(0, 0, 1, 1, 0, 0), [1], None, "rank 1"),
                                    (_LearnOpts(0, 0, 0, 1, 5, 0), [1], None, "max_targets 5"),
                                    (_LearnOpts(0, 0, 0, 1, 0, 3), [1], None, "elim_mode 3"),
                                    (_LearnOpts(0, 0, 0, 1, 0, -1), [1], None, "elim_mode -1")):
        assert call(opts, targets, n) == -1, field  # FW_ERR_ARG
        msg = L.fw_last_error(eng.h).decode()
        assert msg.startswith("fw_learn_neighbors: ") and field in msg, (field, msg)
    assert call(ok, [1], h=None) == -1 and "NULL context" in L.fw_last_error(None).decode()
    # the context is still usable: NULL options mean no feed-forward, one batch, fast_elim
    tg = c["targets"]["pair"]
    assert call(None, tg) == 0
    got = eng._network(ne.value, True)
    check_rows(got, c["full"], tg, 40)
    check_rows(eng.neighbors(tg, round_size=1), c["full"], tg, 40)
    eng.close()
