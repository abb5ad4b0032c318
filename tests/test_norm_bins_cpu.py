"""normalize_data(n_bins=, rank_method=, disc_method=), the parts that need no device: the host front-end against columns worked by
hand from the reference's formulas (preprocessing.jl:238-291), the defaults, the column rule, the refusals, the routing of the options
to whichever front-end runs, and the option validation of csrc/fw_norm_host.h (tests/native/norm_opts_check.cpp, compiled with g++
alone, plainly and under the host sanitizers).  Where a device front-end would run, fw.api.normalize_counts / normalize_abundances
are replaced by recording host stand-ins."""
import inspect
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import engine
from flashweave_jl_amd import preprocess as pre
from tests import api_trace
from tests.norm_mode_tables import dense, host_stand_in
from tests.util import GOLDEN, ROOT

nd = fw.normalize_data
SRC = os.path.join(ROOT, "tests", "native", "norm_opts_check.cpp")
INC = os.path.join(ROOT, "flashweave.jl_amd", "csrc")
BINNED = (dict(test_name="mi_nz"), dict(norm_mode="clr-nonzero-binned"), dict(norm_mode="tss-nonzero-binned"))
NOT_BINNED = (dict(test_name="fz"), dict(test_name="fz_nz"), dict(test_name="mi"), dict(), dict(norm_mode="tss"), dict(norm_mode="clr-adapt"),
              dict(norm_mode="clr-nonzero"), dict(norm_mode="pres-abs"))


@pytest.fixture
def no_device(monkeypatch):
    calls = []

    def record(*a, **kw):
        calls.append((a, kw))
        raise AssertionError("a device front-end was called")
    monkeypatch.setattr(fw.api, "normalize_counts", record)
    monkeypatch.setattr(fw.api, "normalize_abundances", record)
    monkeypatch.setattr(fw.engine, "load_library", record)
    return calls


@pytest.fixture
def recorded(monkeypatch):
    """the two device front-ends as host stand-ins that log (name, number of columns, keywords)"""
    calls = []

    def stand_in(name):
        def front_end(counts, test_name, device=0, **kw):
            calls.append((name, (counts[3] if isinstance(counts, engine.CSC) else np.shape(counts))[1], test_name, kw))
            return host_stand_in(counts, test_name, **kw)
        return front_end
    monkeypatch.setattr(fw.api, "normalize_counts", stand_in("normalize_counts"))
    monkeypatch.setattr(fw.api, "normalize_abundances", stand_in("normalize_abundances"))
    return calls


def tiny():
    rows = [ln.rstrip("\n").split("\t") for ln in open(os.path.join(GOLDEN, "HMP_SRA_gut_tiny.tsv"))]
    return np.array(rows[1:], dtype=np.float64)


def test_the_keywords_exist(no_device):
    """Without the feature n_bins is an unexpected keyword (TypeError)."""
    for f in (nd, pre.normalize, pre.normalize_with_meta, pre.discretize_nz, fw.normalize_counts, fw.normalize_abundances):
        p = inspect.signature(f).parameters
        assert (p["n_bins"].default, p["rank_method"].default, p["disc_method"].default) == (3, "tied", "median"), f
    assert "n_bins" not in inspect.signature(fw.learn_network).parameters  # (the reference's has none either: normalize=False)
    r = nd(api_trace.counts(), test_name="mi_nz", n_bins=4, device_normalize=False)
    assert r["data"].max() <= 3


# ---- columns worked by hand ---------------------------------------------------------------------------------------------------------
def test_tied_and_dense_ranks_at_four_bins():
    # non-zero keys 3 1 2 6 2 5 4: sorted 1 2 2 3 4 5 6; b = 3, step = 1/3 + 1e-5 = 0.33334333...
    #   tied ranks  1 2.5 2.5 4 5 6 7, / 7 = .1429 .3571 .3571 .5714 .7143 .8571 1, / step = 0.43 1.07 1.07 1.71 2.14 2.57 2.99991
    #               -> floor + 1 = 1 2 2 2 3 3 3
    #   dense ranks 1 2 2 3 4 5 6,     / 6 = .1667 .3333 .3333 .5 .6667 .8333 1,    / step = 0.49999 0.99997 0.99997 1.49996 1.99994 2.49993 2.99991
    #               -> floor + 1 = 1 1 1 2 2 3 3
    col = np.array([0, 3, 1, 0, 2, 6, 2, 5, 0, 4], dtype=np.float64)
    tied = pre.discretize_nz(col, col != 0, n_bins=4, rank_method="tied")
    dns = pre.discretize_nz(col, col != 0, n_bins=4, rank_method="dense")
    assert list(tied) == [0, 2, 1, 0, 2, 3, 2, 3, 0, 3]
    assert list(dns) == [0, 2, 1, 0, 1, 3, 1, 3, 0, 2]
    assert list(pre.discretize_nz(col, col != 0, n_bins=4)) == list(tied)  # "tied" and "median" are the defaults
    # the default step at b = 2 is 1/2 + 1e-5, as it always was: ranks 1 2.5 2.5 4 5 6 7 -> / 7 / 0.50001 -> 0 0 0 1 1 1 1
    assert list(pre.discretize_nz(col, col != 0)) == [0, 2, 1, 0, 1, 2, 1, 2, 0, 2]


def test_the_mean_rule_and_its_sum():
    # non-zero keys 4 1 10 3 2: sorted 1 2 3 4 10, padded to 8: ((1 + 2) + (3 + 4)) + ((10 + 0) + (0 + 0)) = 20, / 5 = 4; key <= 4 -> 1, else 2
    col = np.array([4, 0, 1, 10, 0, 3, 2], dtype=np.float64)
    assert pre.pairwise_mean(col[col != 0]) == 4.0
    assert list(pre.discretize_nz(col, col != 0, disc_method="mean")) == [1, 0, 1, 2, 0, 1, 1]
    assert list(pre.discretize_nz(col, col != 0, disc_method="mean", rank_method="dense")) == [1, 0, 1, 2, 0, 1, 1]  # (no ranks in it)
    # the order of the additions is the definition: the tree over the sorted, zero-padded keys, whatever order they come in
    a = np.sort(np.random.default_rng(3).standard_normal(5) * 1e3)
    tree = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + 0.0) + (0.0 + 0.0))
    assert pre.pairwise_mean(a[[3, 0, 4, 2, 1]]) == tree / 5
    assert pre.pairwise_mean(a[[2, 0, 1]]) == ((a[0] + a[1]) + (a[2] + 0.0)) / 3 and pre.pairwise_mean(a[:1]) == a[0]
    assert abs(pre.pairwise_mean(a) - a.mean()) <= 4 * np.spacing(np.abs(a).sum())  # within rounding of the reference's mean


def test_sixty_one_levels():
    # 61 distinct keys at n_bins = 62: b = 61, rank r of 61 -> (r / 61) / (1 / 61 + 1e-5) = r / 1.00061, whose floor is r - 1 for r <= 61: level r
    rng = np.random.default_rng(5)
    keys = rng.permutation(61) * 0.5 + 0.25
    col = np.concatenate([[0.0], keys, [0.0]])
    exp = np.concatenate([[0], np.argsort(np.argsort(keys)) + 1, [0]])
    for rank in ("tied", "dense"):
        got = pre.discretize_nz(col, col != 0, n_bins=62, rank_method=rank)
        assert list(got) == list(exp) and sorted(got[1:-1]) == list(range(1, 62))


# ---- the front-end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [dict(), dict(norm="tss-nonzero-binned")], ids=["clr", "tss"])
def test_the_defaults_are_the_call_without_options(mode):
    x = tiny()
    plain = pre.normalize(x, "mi_nz", **mode)
    spelled = pre.normalize(x, "mi_nz", n_bins=3, rank_method="tied", disc_method="median", **mode)
    assert plain[0].shape[1] > 5 and plain[0].dtype == spelled[0].dtype
    for a, b in zip(plain, spelled):
        assert np.array_equal(a, b)


def _column_rule_table():
    """16 samples x 5 columns.  Column 3 gives every sample a second count, so that the TSS keys of the others are what is written
    here; column 4 is constant and leaves before the sums.  The keys x / (x + column 3):
      column 0, samples 0-5:   1/7 2/8 3/9 4/10 5/11 6/12   six distinct keys
      column 1, samples 6-11:  1/2 1/2 1/2 3/4 3/4 3/4      two distinct keys
      column 2, samples 12-15: 2/4 four times               one key"""
    x = np.zeros((16, 5), dtype=np.int64)
    x[:, 4] = 9
    x[:6, 0], x[:6, 3] = [1, 2, 3, 4, 5, 6], 6
    x[6:12, 1], x[6:12, 3] = [1, 1, 1, 3, 3, 3], 1
    x[12:, 2], x[12:, 3] = 2, 2
    return x


def test_a_column_with_fewer_levels_than_bins_is_dropped():
    """The rule: a column stays iff its non-zero entries show exactly n_bins - 1 distinct levels (preprocessing.jl:511-515).
    n_bins = 4 (step 0.33334): column 0, tied ranks 1 .. 6 of 6 -> levels 1 1 2 2 3 3: kept; column 1, ranks 2 2 2 5 5 5 of 5 -> 0.4 and
    1 -> levels 2 and 3, two of three: dropped.  n_bins = 3 (step 0.50001): column 1 -> levels 1 and 2: kept.  Column 2 has one level."""
    x = _column_rule_table()
    for opts in (dict(n_bins=4), dict(n_bins=4, rank_method="dense"), dict(n_bins=3), dict(disc_method="mean")):
        data, row_mask, col_mask = pre.normalize(x, "mi_nz", norm="tss-nonzero-binned", **opts)
        b = opts.get("n_bins", 3) - 1
        filt = x[:, :4]  # (the constant column goes first)
        nzm = filt != 0
        keys = pre.tss(filt.astype(np.float64)).astype(np.float64)
        levels = np.stack([pre.discretize_nz(keys[:, j], nzm[:, j], **opts) for j in range(4)], axis=1)
        keep = [len(set(levels[nzm[:, j], j])) == b for j in range(4)]
        assert list(col_mask) == keep + [False] and row_mask.all()
        assert np.array_equal(data, levels[:, keep]) and data.max() == b
        assert col_mask[0] and not col_mask[2]
    at4 = pre.normalize(x, "mi_nz", norm="tss-nonzero-binned", n_bins=4)
    assert list(at4[2][:3]) == [True, False, False] and list(at4[0][:6, 0]) == [1, 1, 2, 2, 3, 3]
    at3 = pre.normalize(x, "mi_nz", norm="tss-nonzero-binned")
    assert list(at3[2][:3]) == [True, True, False] and list(at3[0][6:12, 1]) == [1, 1, 1, 2, 2, 2]


def test_meta_variables_stay_in_two_bins(no_device):
    x = api_trace.counts(8, 0, 12)
    meta = np.stack([np.arange(12) % 2, 0.5 + 0.25 * np.arange(12)], axis=1).astype(np.float64)
    r = nd(x, test_name="mi_nz", n_bins=4, meta_data=meta, make_onehot=False, device_normalize=False)
    got = r["data"][:, r["meta_mask"]]
    assert got.shape[1] == 2 and np.array_equal(got[:, 1], pre.discretize(meta[:, 1], 2)) and set(got[:, 1]) == {0, 1}
    otu = pre.normalize(x, "mi_nz", n_bins=4)[0]
    assert np.array_equal(r["data"][:, ~r["meta_mask"]], otu)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_device_call(no_device):
    x = api_trace.counts()
    tables = (x, sp.csc_matrix(x))
    for table in tables:
        for mode in BINNED:
            for bad in (2, 1, 0, -3, 63, 100, 4.0, "4", None, True):
                with pytest.raises(ValueError, match="n_bins"):
                    nd(table, n_bins=bad, **mode)
            with pytest.raises(ValueError, match="rank_method"):
                nd(table, rank_method="average", **mode)
            with pytest.raises(ValueError, match="disc_method"):
                nd(table, disc_method="quantile", **mode)
            for n_bins in (4, 62):
                with pytest.raises(ValueError, match="disc_method.*n_bins"):
                    nd(table, disc_method="mean", n_bins=n_bins, **mode)
        for mode in NOT_BINNED:
            for opt, name in ((dict(n_bins=4), "n_bins"), (dict(rank_method="dense"), "rank_method"), (dict(disc_method="mean"), "disc_method")):
                with pytest.raises(ValueError, match=name):
                    nd(table, **opt, **mode)
                with pytest.raises(ValueError, match=name):
                    nd(table, abundances=True, **opt, **mode)
    # the front-ends of their own refuse the same, before the library is loaded
    for f in (fw.normalize_counts, fw.normalize_abundances, pre.normalize):
        for opt, name in ((dict(n_bins=2), "n_bins"), (dict(n_bins=63), "n_bins"), (dict(rank_method="min"), "rank_method"),
                          (dict(disc_method="kmeans"), "disc_method"), (dict(disc_method="mean", n_bins=5), "disc_method")):
            with pytest.raises(ValueError, match=name):
                f(x, "mi_nz", **opt)
        for test_name in ("fz", "fz_nz", "mi"):
            with pytest.raises(ValueError, match="rank_method"):
                f(x, test_name, rank_method="dense")
        with pytest.raises(ValueError, match="n_bins"):
            f(x, "fz", norm="tss", n_bins=5)
    with pytest.raises(ValueError, match="n_bins"):
        pre.normalize_with_meta(x, "fz_nz", np.ones((6, 1)), make_onehot=False, n_bins=4)
    assert no_device == []


# ---- routing ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("abundances", [False, True])
def test_options_reach_the_front_end_as_keywords(form, abundances, recorded):
    wrap = sp.csc_matrix if form == "sparse" else np.asarray
    main, e1, e2 = api_trace.counts(8, 0, 12), api_trace.counts(4, 2, 12), api_trace.counts(3, 5, 12)
    name = "normalize_abundances" if abundances else "normalize_counts"
    opts = dict(n_bins=4, rank_method="dense")
    r = nd(wrap(main), test_name="mi_nz", extra_data=[(wrap(e1), None), (wrap(e2), None)], abundances=abundances, **opts)
    assert recorded == [(name, 8, "mi_nz", opts), (name, 4, "mi_nz", opts), (name, 3, "mi_nz", opts)]  # every table, the same options
    exp = np.concatenate([pre.normalize(t, "mi_nz", **opts)[0] for t in (e2, e1, main)], axis=1)
    assert np.array_equal(dense(r["data"]), exp)
    del recorded[:]
    nd(wrap(main), norm_mode="tss-nonzero-binned", disc_method="mean", abundances=abundances)
    assert recorded == [(name, 8, "mi_nz", dict(norm="tss-nonzero-binned", disc_method="mean"))]  # only what is away from its default
    del recorded[:]
    nd(wrap(main), test_name="mi_nz", n_bins=3, rank_method="tied", disc_method="median", abundances=abundances,
       extra_data=[(wrap(e1), None)])
    assert recorded == [(name, 8, "mi_nz", {}), (name, 4, "mi_nz", {})]  # the defaults add no keyword
    del recorded[:]
    mask = np.r_[np.zeros(8, bool), True]
    table = np.concatenate([main, (np.arange(12) % 2)[:, None]], axis=1)
    r = nd(wrap(table), test_name="mi_nz", meta_mask=mask, abundances=abundances, **opts)
    assert recorded == [(name, 8, "mi_nz", opts)] and list(r["meta_mask"][-1:]) == [True]


def test_the_engine_front_ends_pick_the_opts_entry_points(monkeypatch):
    """At the defaults the entry points without options are called with the arguments they always got; away from them, the *_opts
    siblings, with the options as keywords for the binding."""
    seen = []

    class Lib:
        pass
    for name in ("fw_normalize_counts", "fw_normalize_counts_csc", "fw_normalize_abund", "fw_normalize_abund_csc"):
        setattr(Lib, name, name)
        setattr(Lib, name + "_opts", name + "_opts")
    monkeypatch.setattr(fw.engine, "load_library", lambda: Lib)
    monkeypatch.setattr(fw.engine, "_normalize_dense", lambda fe, x, t, d, **kw: seen.append((fe, kw)))
    monkeypatch.setattr(fw.engine, "_normalize_csc", lambda fe, who, triple, t, d, **kw: seen.append((fe, kw)))
    x = api_trace.counts()
    opts = dict(n_bins=7, rank_method="dense")
    for f, stem, table in ((fw.normalize_counts, "fw_normalize_counts", x), (fw.normalize_abundances, "fw_normalize_abund", x / 4.0)):
        f(table, "mi_nz")
        f(sp.csc_matrix(table), "mi_nz", n_bins=3, rank_method="tied", disc_method="median")
        f(table, "mi_nz", **opts)
        f(sp.csc_matrix(table), "mi_nz", norm="tss-nonzero-binned", disc_method="mean")
        assert seen == [(stem, {}), (stem + "_csc", {}), (stem + "_opts", opts),
                        (stem + "_csc_opts", dict(norm="tss-nonzero-binned", disc_method="mean"))]
        del seen[:]


def test_the_options_struct_mirrors_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "flashweave_amd.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %d %d %d %d\\n", sizeof(fw_norm_opts), offsetof(fw_norm_opts, n_bins), offsetof(fw_norm_opts, rank_method),\n'
                   'offsetof(fw_norm_opts, disc_method), FW_RANK_TIED, FW_RANK_DENSE, FW_DISC_MEDIAN, FW_DISC_MEAN);\nreturn 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    out = [int(t) for t in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    C = engine._NormOpts
    assert out[:4] == [engine.C.sizeof(C), C.n_bins.offset, C.rank_method.offset, C.disc_method.offset] == [12, 0, 4, 8]
    assert out[4:] == [engine.FW_RANK["tied"], engine.FW_RANK["dense"], engine.FW_DISC["median"], engine.FW_DISC["mean"]]


# ---- the native validation ----------------------------------------------------------------------------------------------------------
def _compile(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", INC, "-o", exe, SRC], check=True)
    return exe


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), r.stdout[-2000:] + r.stderr[-3000:]
    return [ln.split(" ") for ln in r.stdout.splitlines()[:-1]]


KINDS_BINNED = (engine.FW_MI_NZ, engine.FW_NORM_TSS_BINNED)
KINDS_OTHER = (engine.FW_FZ, engine.FW_FZ_NZ, engine.FW_MI, engine.FW_NORM_TSS)


def _native_cases():
    """[(command line, expected answer: ("ok", b, dense, mean, plain) or the field a refusal must name)]"""
    cases = []
    for kind in KINDS_BINNED + KINDS_OTHER:
        cases.append(("null %d" % kind, ("ok", 2, 0, 0, 1)))
        cases.append(("opts %d 3 0 0" % kind, ("ok", 2, 0, 0, 1)))  # the defaults, spelled out: every kind takes them
        for bad in (2, 0, -1, 63, 1 << 20):
            cases.append(("opts %d %d 0 0" % (kind, bad), "n_bins"))
        for bad in (-1, 2):
            cases.append(("opts %d 3 %d 0" % (kind, bad), "rank_method"))
            cases.append(("opts %d 3 0 %d" % (kind, bad), "disc_method"))
        cases.append(("opts %d 4 0 1" % kind, "disc_method"))
        cases.append(("opts %d 62 1 1" % kind, "disc_method"))
    for kind in KINDS_BINNED:
        for n_bins in (3, 4, 7, 62):
            for rank in (0, 1):
                cases.append(("opts %d %d %d 0" % (kind, n_bins, rank), ("ok", n_bins - 1, rank, 0, int(n_bins == 3 and rank == 0))))
        for rank in (0, 1):
            cases.append(("opts %d 3 %d 1" % (kind, rank), ("ok", 2, rank, 1, 0)))
    for kind in KINDS_OTHER:
        cases += [("opts %d 4 0 0" % kind, "n_bins"), ("opts %d 3 1 0" % kind, "rank_method"), ("opts %d 3 0 1" % kind, "disc_method")]
    return cases


def _check_native(exe):
    cases = _native_cases()
    out = _run(exe, "".join(c + "\n" for c, _ in cases))
    assert len(out) == len(cases)
    for (cmd, exp), got in zip(cases, out):
        if isinstance(exp, tuple):
            assert got == [str(v) for v in exp], (cmd, got)
        else:
            assert got[0] == "refused" and got[1] == exp, (cmd, got)  # the words begin with the field's name


def test_native_option_validation(tmp_path):
    _check_native(_compile(tmp_path, "norm_opts_check", []))


def test_native_option_validation_under_host_sanitizers(tmp_path):
    # host code only, a stand-alone program.  The flags must compile, link and start a trivial program here; otherwise the leg is skipped
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
    _check_native(_compile(tmp_path, "norm_opts_check_san", flags))
