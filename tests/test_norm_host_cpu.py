"""The host rules of the device normalisation front-end (csrc/fw_norm_host.h) without a device: which samples and columns survive and
with which parameters.  tests/native/norm_host_check.cpp calls the header on what this file hands it -- per-row totals computed with
numpy, as C99 hex floats -- and prints what came back; it is compiled with g++ alone, plainly and under the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from flashweave_jl_amd import engine
from flashweave_jl_amd import preprocess as pre
from tests.util import ROOT

SRC = os.path.join(ROOT, "tests", "native", "norm_host_check.cpp")
INC = os.path.join(ROOT, "flashweave.jl_amd", "csrc")
FW_FZ, FW_FZ_NZ = engine.FW_FZ, engine.FW_FZ_NZ
# both sides evaluate the same Float64 expressions on the same inputs and differ in a few libm calls of a few ulp each; the arguments
# of exp are bounded by 745 in magnitude, so pseudo and g deviate relatively by less than about 745 * 4 * 2^-53 = 3.3e-13, and the
# logarithm carries that over as an absolute error
ATOL = 1e-11


def _compile(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *extra, "-I", INC, "-o", exe, SRC], check=True)
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _compile(tmp_path_factory.mktemp("norm_host"), "norm_host_check", [])


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=np.float64).ravel())


def _run(exe, text):
    """the program on `text` -> its output lines but the closing ok, each as [name, token, ...]"""
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.endswith("ok\n"), r.stdout[-2000:] + r.stderr[-3000:]
    return [ln.split(" ") for ln in r.stdout.splitlines()[:-1]]


def _floats(line):
    return np.array([float.fromhex(t) for t in line[1:]], dtype=np.float64)


def _totals(M):
    """per-row totals of a table whose columns are all kept: S, SL, NZ, RMIN"""
    M = np.asarray(M, dtype=np.float64)
    present = M != 0
    SL = np.array([np.log(M[i, present[i]]).sum() for i in range(M.shape[0])])
    RMIN = np.array([M[i, present[i]].min() if present[i].any() else np.inf for i in range(M.shape[0])])
    return M.sum(axis=1), SL, M.shape[1] - present.sum(axis=1), RMIN


def _params_text(kind, totals, pk, tie_rel, s32=None):
    S, SL, NZ, RMIN = totals
    cols = [S, SL, NZ, RMIN] + ([s32] if s32 is not None else [])
    rows = "\n".join(_hex([c[i] for c in cols]) for i in range(len(S)))
    return "params %d %d %d %s %d\n%s\n" % (kind, len(S), pk, float(tie_rel).hex(), s32 is not None, rows)


def _params(exe, kind, M, tie_rel=0.0, totals=None):
    """norm_row_params on the totals of M -> (mask, rows, pseudo, g), or the refusal's line"""
    out = _run(exe, _params_text(kind, totals or _totals(M), np.shape(M)[1], tie_rel))
    if out[0][0] == "refused":
        return out[0]
    mask, rows, pseudo, g = (_floats(ln) for ln in out)
    return mask.astype(bool), rows.astype(int), pseudo, g


def _counts():
    x = np.random.default_rng(11).integers(0, 30, size=(23, 19)).astype(np.float64)
    x[x < 12] = 0
    x[:, 0] += 1  # every sample has reads
    x[7] = x[2]  # two samples of one depth
    return x


def _relative():
    x = _counts()
    return x / x.sum(axis=1, keepdims=True)  # every sample of depth 1 up to rounding


def _underflow():
    x = _relative()
    x[5, 1:] = 0
    x[5, 0] = 1e-300  # the table's smallest value: the floor is 1e-301, and the pseudo-count of this sample (and of others) underflows
    return x


@pytest.mark.parametrize("tie_anchor", [False, True])
@pytest.mark.parametrize("table", [_counts, _relative, _underflow], ids=["counts", "relative", "underflow"])
def test_kept_samples_and_clr_adapt_values_are_adaptive_clrs(exe, table, tie_anchor):
    M = table()
    width = M.shape[1]
    ref, kept = pre.adaptive_clr(M, tie_anchor=tie_anchor)
    mask, rows, pseudo, g = _params(exe, FW_FZ, M, tie_rel=width * 2.0 ** -52 if tie_anchor else 0.0)
    assert np.array_equal(mask, kept) and np.array_equal(rows, np.flatnonzero(kept))
    assert kept.all() if table is not _underflow else (kept.any() and not kept[5])  # the underflow: dropped, its mask bit cleared
    filled = np.where(M[rows] != 0, M[rows], pseudo[:, None])
    got = np.log(filled / g[:, None])
    print("largest deviation of clr_adapt from adaptive_clr:", np.abs(got - ref).max())
    assert np.allclose(got, ref, rtol=0, atol=ATOL)


def test_geometric_mean_of_the_non_zeros(exe):
    M = _counts()
    M[4, 1:] = 0  # one OTU: g is its count, the clr_nz value 0
    mask, rows, pseudo, g = _params(exe, FW_FZ_NZ, M)
    assert mask.all() and np.array_equal(rows, np.arange(len(M))) and not pseudo.any()
    got = np.where(M != 0, np.log(np.where(M != 0, M, 1.0) / g[:, None]), 0.0)
    print("largest deviation of clr_nz:", np.abs(got - pre.clr_nz(M)).max())
    assert np.allclose(got, pre.clr_nz(M), rtol=0, atol=ATOL)
    for kind in (engine.FW_MI, engine.FW_NORM_TSS):  # no geometric mean: 1
        assert np.array_equal(_params(exe, kind, M)[3], np.ones(len(M)))


def _pseudo_with_anchor(totals, pk, md):
    S, SL, NZ, RMIN = totals
    base = 1.0 if RMIN.min() >= 1 else RMIN.min() / 10
    return np.exp((1.0 / (NZ - pk)) * ((NZ[md] - pk) * np.log(base) + SL[md] - SL))


def test_anchor_rule(exe):
    # counts (tie_rel = 0): the first sample of maximal sum is the anchor -- samples 2 and 7 are equal, so make 7 differ in its zeros
    M = _counts()
    M[2] *= 50
    M[7] = 0
    M[7, 0] = M[2].sum()  # the same depth in one count
    totals = _totals(M)
    assert totals[0][2] == totals[0][7] == totals[0].max()
    first, second = _pseudo_with_anchor(totals, M.shape[1], 2), _pseudo_with_anchor(totals, M.shape[1], 7)
    assert not np.allclose(first, second, rtol=1e-3)
    assert np.allclose(_params(exe, FW_FZ, M)[2], first, rtol=1e-12, atol=0)
    # real values: an earlier sample whose sum lies inside the pk * 2^-52 window takes over; outside it (or with tie_rel = 0) it does not
    pk = 8
    for s0, inside in ((1.0 - 2.0 ** -53, True), (1.0 - pk * 2.0 ** -51, False)):
        totals = (np.array([s0, 1.0, 0.5]), np.array([-9.0, -4.0, -6.0]), np.array([2, 5, 3]), np.array([0.01, 0.02, 0.03]))
        M = np.zeros((3, pk))
        for tie_rel, anchor in ((pk * 2.0 ** -52, 0 if inside else 1), (0.0, 1)):
            got = _params(exe, FW_FZ, M, tie_rel=tie_rel, totals=totals)[2]
            assert np.allclose(got, _pseudo_with_anchor(totals, pk, anchor), rtol=1e-12, atol=0), (s0, tie_rel)
        assert not np.allclose(_pseudo_with_anchor(totals, pk, 0), _pseudo_with_anchor(totals, pk, 1), rtol=1e-3)


def test_samples_without_reads_and_the_tss_divisors(exe):
    M = _counts()
    M[[3, 20]] = 0
    totals = _totals(M)
    mask, rows, _, _ = _params(exe, engine.FW_MI, M)
    assert np.array_equal(mask, M.sum(axis=1) > 0) and np.array_equal(rows, np.flatnonzero(mask))
    assert _params(exe, FW_FZ, np.zeros((3, 4)))[1:] == ["-1", "no", "sample", "has", "reads"]
    s32 = M.sum(axis=1).astype(np.float32)
    pk = M.shape[1]
    assert _run(exe, _params_text(engine.FW_NORM_TSS, totals, pk, 0.0, s32))[0][0] == "mask"  # (a dropped sample's sum of 0 is not looked at)
    for i, value, word in ((6, 0.0, "zero"), (9, np.inf, "infinite")):
        bad = s32.copy()
        bad[i] = value
        assert _run(exe, _params_text(engine.FW_NORM_TSS_BINNED, totals, pk, 0.0, bad))[0] == ["refused", str(i), word]


def test_chunk_reduction_is_a_loop_in_chunk_order(exe):
    n, rng = 37, np.random.default_rng(5)
    rsum, rlog = rng.random((64, n)) * 1e6, rng.standard_normal((64, n)) * 30
    rzero, rmin = rng.integers(0, 1000, size=(64, n)), rng.random((64, n))
    rmin[:, 4] = np.inf
    out = _run(exe, "reduce %d\n%s\n%s\n%s\n%s\n" % (n, _hex(rsum), _hex(rlog), _hex(rzero), _hex(rmin)))
    S, SL = np.zeros(n), np.zeros(n)
    for c in range(64):  # the same additions in the same order: to the bit
        S, SL = S + rsum[c], SL + rlog[c]
    for got, exp in zip(out, (S, SL, rzero.sum(axis=0), rmin.min(axis=0))):
        assert np.array_equal(_floats(got), exp.astype(np.float64)), got[0]


def test_column_helper(exe):
    cols = np.array([1, 2, 5, 6, 9, 11])
    for two in ([1, 0, 1, 1, 0, 1], [0, 0, 0, 0, 0, 1], [1] * 6, [0] * 6):
        two = np.array(two, dtype=bool)
        sel, kept, mask = (_floats(ln).astype(int) for ln in _run(exe, "keep 6 12\n%s\n%s\n" % (_hex(two), _hex(cols))))
        assert np.array_equal(sel, np.flatnonzero(two)) and np.array_equal(kept, cols[two])
        exp = np.ones(12, dtype=int)
        exp[cols[~two]] = 0  # exactly the dropped columns' bits
        assert np.array_equal(mask, exp)
        assert (len(sel) == 0) == (not two.any())  # "none left"


def test_rownew_and_output_colptr_are_cumsums(exe):
    mask = np.array([1, 0, 0, 1, 1, 0, 1, 1, 0], dtype=bool)
    rows = np.flatnonzero(mask)
    got = _floats(_run(exe, "rownew %d %d\n%s\n" % (len(mask), len(rows), _hex(rows)))[0]).astype(int)
    assert np.array_equal(got, np.where(mask, np.cumsum(mask) - 1, -1))
    lengths = np.array([3, 0, 7, 1, 4, 0, 2])
    colptr, fcols = np.concatenate(([0], np.cumsum(lengths))), np.array([0, 2, 3, 6])
    got = _floats(_run(exe, "ocolptr %d %d\n%s\n%s\n" % (len(lengths), len(fcols), _hex(colptr), _hex(fcols)))[0]).astype(int)
    assert np.array_equal(got, np.concatenate(([0], np.cumsum(lengths[fcols]))))
    assert np.array_equal(_floats(_run(exe, "ocolptr %d 0\n%s\n" % (len(lengths), _hex(colptr)))[0]), [0])


def test_kind_description_agrees_with_the_engines_table(exe):
    kinds = {int(ln[1]): ln[2:] for ln in _run(exe, "kinds\n")}
    assert sorted(kinds) == sorted(engine.NORM_OUT_DTYPE) + [9]
    assert kinds[9][0] == "0"  # unknown
    for kind, dtype in engine.NORM_OUT_DTYPE.items():
        known, i32, tss, binned = (t == "1" for t in kinds[kind][:4])
        assert known and i32 == (dtype is np.int32)
        assert tss == (kind in engine._NORMS.values()) and binned == (kind in (engine.FW_MI_NZ, engine.FW_NORM_TSS_BINNED))
    # the modes the two kernels take, with the values they always had
    assert [kinds[k][4] for k in (engine.FW_FZ, engine.FW_FZ_NZ)] == ["0", "1"]
    assert [kinds[k][5] for k in (engine.FW_MI, engine.FW_MI_NZ, engine.FW_NORM_TSS_BINNED, engine.FW_FZ_NZ, engine.FW_NORM_TSS)] == list("01123")
    assert " ".join(kinds[engine.FW_MI][6:]) == "no column with two levels"
    assert " ".join(kinds[engine.FW_MI_NZ][6:]) == " ".join(kinds[engine.FW_NORM_TSS_BINNED][6:]) == "no column whose non-zero abundances fall into two bins"


def test_under_host_sanitizers(tmp_path):
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
    san = _compile(tmp_path, "norm_host_check_san", flags)
    text = "kinds\n" + "".join(_params_text(k, _totals(M), M.shape[1], t) for k in (FW_FZ, FW_FZ_NZ) for M, t in ((_counts(), 0.0), (_relative(), 19 * 2.0 ** -52)))
    s32 = _counts().sum(axis=1).astype(np.float32)
    text += _params_text(engine.FW_NORM_TSS, _totals(_counts()), 19, 0.0, s32) + _params_text(FW_FZ, _totals(np.zeros((3, 4))), 4, 0.0)
    rng = np.random.default_rng(6)
    text += "reduce 5\n%s\n%s\n%s\n%s\n" % tuple(_hex(rng.integers(0, 9, size=(64, 5))) for _ in range(4))
    text += "keep 3 4\n%s\n%s\nkeep 2 2\n%s\n%s\n" % (_hex([0, 1, 0]), _hex([0, 2, 3]), _hex([0, 0]), _hex([0, 1]))
    text += "rownew 4 2\n%s\nrownew 3 0\nocolptr 3 2\n%s\n%s\nocolptr 1 0\n%s\n" % (_hex([1, 3]), _hex([0, 2, 2, 5]), _hex([0, 2]), _hex([0, 4]))
    _run(san, text)
