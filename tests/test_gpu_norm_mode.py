"""The two total-sum-scaling modes of the device front-end (fw_normalize_counts* / fw_normalize_abund* with FW_NORM_TSS /
FW_NORM_TSS_BINNED, csrc/fw_norm.hip) against the host front-end (preprocess.normalize(norm=...), pinned on the reference's
fixtures in tests/test_norm_mode_cpu.py) and against the fixtures themselves.  Every comparison is bit for bit: the arithmetic is
Float32 additions in a fixed order and one IEEE division per cell, no libm call, so nothing is left to a tolerance."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import preprocess as pre
from tests.norm_mode_tables import TSS_MODES, bits, dense, edge_table, f32_sum_left_to_right, fixture, hmp

pytestmark = pytest.mark.gpu
FAMILY = pre.TSS_NORMS  # the test_name a norm goes with


@functools.lru_cache(maxsize=None)
def host(table, mode):
    """the host front-end's answer for one of the tables below, computed once"""
    return pre.normalize(TABLES[table](), FAMILY[mode], norm=mode)


def real_table():
    """edge_table's shape with non-integral values: samples 20 / 21 differ as Float64 and are equal as Float32 (their quotients
    tie), sample 40 holds 2^90 and 2^-40 (the quotient 2^-130 is a Float32 subnormal); the constant column holds a dyadic value,
    so that the host's floating-point variance of it is exactly 0 like the device's min == max."""
    y = edge_table().astype(np.float64) * 0.37
    y[20], y[21] = 0, 0
    y[20, [0, 1]] = (0.3, 0.6)
    y[21, [0, 1]] = (0.3 * (1 + 2.0 ** -40), 0.6 * (1 + 2.0 ** -40))
    y[40] = 0
    y[40, [0, 1]] = (2.0 ** 90, 2.0 ** -40)
    y[:, 5] = 0.5
    return y


def tall_table(n=16_500):
    """n x 3 with every sample present in column 0: more than NORM_BIN_MAX = 16 384 sort keys per column, dense and CSC, and long
    runs of tied quotients (the pattern repeats every 1 155 samples)"""
    i = np.arange(n)
    return np.stack([1 + i % 7, (i * i) % 5, (i % 3 == 0) * (1 + i % 11)], axis=1).astype(np.int64)


TABLES = {"edge": edge_table, "real": real_table, "tall": tall_table, "hmp": hmp}


def same(got, exp, sparse=False):
    """(data, row_mask, col_mask) of a device front-end against the expected triple, to the bit; a sparse result holds one entry
    per present value of the kept block"""
    assert np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    assert sp.issparse(got[0]) is sparse and got[0].shape == exp[0].shape and got[0].dtype == exp[0].dtype
    assert np.array_equal(bits(dense(got[0])), bits(dense(exp[0])))


def test_the_edge_table_is_what_it_says():
    x = edge_table()
    assert x.shape == (257, 130) and (x[:, 5] == 4).all() and not x[[9, 200]][:, np.arange(130) != 5].any()
    kept = np.nonzero(x.min(axis=0) != x.max(axis=0))[0]
    assert kept[0] == 0 and 5 not in kept and len(kept) > 64
    row = x[30, kept].astype(np.float64)
    s = f32_sum_left_to_right(row)  # 2^24, then ones that are each rounded away
    assert s == np.float32(2.0 ** 24) and s != np.float32(row.sum()) and s != f32_sum_left_to_right(row[::-1])
    exp, rm, cm = host("edge", "tss")
    assert not cm[5] and not rm[9] and not rm[200] and rm.sum() == 255
    r = np.cumsum(rm) - 1
    assert exp[r[30], 0] == 1.0 and exp[r[20], 0] == exp[r[21], 0] == np.float32(1) / np.float32(3)  # the tie the binning must keep


@pytest.mark.parametrize("mode", TSS_MODES)
def test_dense_counts_against_the_host(mode):
    x = edge_table()
    got = fw.normalize_counts(x, FAMILY[mode], norm=mode)
    same(got, host("edge", mode))
    if mode == "tss":  # the constant column entered no sum: every kept sample sums to 1 (sample 30 aside, whose ones were rounded away)
        sums = got[0].astype(np.float64).sum(axis=1)
        assert np.allclose(np.delete(sums, (np.cumsum(got[1]) - 1)[30]), 1.0, atol=1e-5)
    else:
        assert set(np.unique(got[0])) == {0, 1, 2}
    same(fw.normalize_counts(sp.csc_matrix(x), FAMILY[mode], norm=mode), tuple(got), sparse=True)  # the CSC form of the same table
    csc = fw.normalize_counts(sp.csc_matrix(x), FAMILY[mode], norm=mode)[0]
    assert csc.nnz == int((x[got[1]][:, got[2]] != 0).sum())


@pytest.mark.parametrize("mode", TSS_MODES)
def test_float64_values(mode):
    x = edge_table()
    counts = fw.normalize_counts(x, FAMILY[mode], norm=mode)
    same(fw.normalize_abundances(x.astype(np.float64), FAMILY[mode], norm=mode), counts)  # integers: the bits of the count path
    same(fw.normalize_abundances(sp.csc_matrix(x.astype(np.float64)), FAMILY[mode], norm=mode), counts, sparse=True)
    y, exp = real_table(), host("real", mode)
    assert exp[1][40] and not exp[2][5]
    got = fw.normalize_abundances(y, FAMILY[mode], norm=mode)
    if mode == "tss":
        r = np.cumsum(exp[1]) - 1
        assert exp[0][r[40], 1] == np.float32(2.0 ** -130)  # a subnormal: the build must not flush it
        print("subnormal quotient: host %r device %r" % (exp[0][r[40], 1], got[0][r[40], 1]))
        assert np.array_equal(bits(exp[0][r[20], :2]), bits(exp[0][r[21], :2]))  # equal as Float32
    same(got, exp)
    same(fw.normalize_abundances(sp.csc_matrix(y), FAMILY[mode], norm=mode), exp, sparse=True)


@pytest.mark.parametrize("mode", TSS_MODES)
def test_the_reference_fixtures_through_the_device(mode):
    exp = fixture(mode)
    for table in (hmp(), sp.csc_matrix(hmp())):
        got, rm, cm = fw.normalize_counts(table, FAMILY[mode], norm=mode)
        assert got.shape == (346, 50) and rm.sum() == 346 and cm.all() and got.dtype == exp.dtype
        assert np.array_equal(bits(dense(got)), bits(exp))


def test_binned_keys_beyond_the_lds():
    x, exp = tall_table(), host("tall", "tss-nonzero-binned")
    assert exp[0].shape == (16_500, 3) and (x[:, 0] != 0).sum() > 16_384
    same(fw.normalize_counts(x, "mi_nz", norm="tss-nonzero-binned"), exp)
    same(fw.normalize_counts(sp.csc_matrix(x), "mi_nz", norm="tss-nonzero-binned"), exp, sparse=True)


@pytest.mark.parametrize("mode", TSS_MODES)
def test_the_entry_points_refuse_a_row_sum_that_is_no_divisor(mode):
    """Past the Python refusals (the C ABI has other callers): a kept sample whose Float32 sum is 0 -- its only value vanishes as a
    Float32 -- or infinite is FW_ERR_ARG from the entry point, dense and CSC, and names the sample."""
    L = fw.load_library()
    for values, word in (((2.0 ** -160, 0.0), "zero"), ((2.0 ** 127, 2.0 ** 127), "infinite")):
        y = np.asfortranarray(real_table()[:, :8])
        y[40, :2] = values
        with pytest.raises(fw.FlashWeaveError, match="sample 40 is %s" % word):
            fw.engine._normalize_dense(L.fw_normalize_abund, y, FAMILY[mode], 0, norm=mode)
        with pytest.raises(fw.FlashWeaveError, match="sample 40 is %s" % word):
            fw.engine._normalize_csc(L.fw_normalize_abund_csc, "test", fw.engine.as_csc(sp.csc_matrix(y), np.float64), FAMILY[mode], 0, norm=mode)


def test_normalize_data_then_learn_network():
    i = np.arange(351)
    table = np.concatenate([hmp(), np.stack([i % 2, 0.5 + 0.25 * (i % 7)], axis=1)], axis=1)  # a 0 / 1 column and a covariate, marked
    mask = np.r_[np.zeros(50, bool), True, True]
    on_dev = fw.normalize_data(table, norm_mode="tss-nonzero-binned", meta_mask=mask)
    on_host = fw.normalize_data(table, norm_mode="tss-nonzero-binned", meta_mask=mask, device_normalize=False)
    assert np.array_equal(on_dev["data"], on_host["data"]) and on_dev["data"].dtype == on_host["data"].dtype == np.int32
    assert on_dev["header"] == on_host["header"] and list(on_dev["meta_mask"]) == [False] * 50 + [True] * 2
    assert np.array_equal(on_dev["data"][:, :50], fixture("tss-nonzero-binned"))
    nets = [fw.learn_network(r["data"], normalize=False, sensitive=False, heterogeneous=True, meta_mask=r["meta_mask"], header=r["header"])
            for r in (on_dev, on_host)]
    assert nets[0]["edges"] == nets[1]["edges"] and nets[0]["variable_ids"] == nets[1]["variable_ids"]
