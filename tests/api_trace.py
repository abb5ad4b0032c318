"""Call traces of learn_network / normalize_data without a device: a helper module, not a test (tests/test_api_trace_cpu.py compares
what it returns with tests/golden/api_trace.json).  It uses the public surface only -- fw.learn_network, fw.normalize_data and the two
names the other CPU tests replace on the module, fw.api.Engine and fw.api.normalize_counts -- so the same file runs on any commit:
the golden file is recorded on the PARENT of a change to api.py (`python -m tests.api_trace --write` in a checkout of the parent with
this file copied in), never on the code under test.

A case is one call.  Its trace holds the calls the recording engine and the stand-in front-end saw (constructor arguments, what
set_data received, compute_cor, the keywords of lgl, close), the result or the exception's type and full message, and every warning
with its category, its message and whether it was attributed to THIS file -- the caller of learn_network; that flag pins the
warning's stacklevel.  Arrays are recorded by shape, dtype and values (integers and booleans exactly, floats to np.allclose(rtol=1e-6,
atol=1e-7): a digest of float bytes would tie the golden to one libm), a sparse matrix as its three arrays.  The tables are built by
integer arithmetic, not by a random generator, and are at most 6 x 8.  The golden file folds what repeats (pack / unpack): an array
that occurs in many traces is stored once, the dicts that repeat from case to case as what differs from the first case's."""
import json
import os
import pathlib
import sys
import tempfile
import types
import warnings

import numpy as np
import scipy.sparse as sp

import flashweave_jl_amd as fw
from flashweave_jl_amd import io as fio
from flashweave_jl_amd import preprocess as pre
from flashweave_jl_amd.engine import CSC

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "api_trace.json")
KINDS = {"fz": dict(sensitive=True, heterogeneous=False), "fz_nz": dict(sensitive=True, heterogeneous=True),
         "mi": dict(sensitive=False, heterogeneous=False), "mi_nz": dict(sensitive=False, heterogeneous=True)}
EDGES = {(0, 1): 0.5, (1, 3): -1.25}
REJECTIONS = {0: {2: ((1, 3), (1.5, 0.25, 0, True), (3, 0.5))}}
_LOG = []


def _scatter(colptr, rowval, nzval, shape):
    """a CSC triple as a dense matrix, without scipy's toarray (test_the_split_never_densifies_the_table patches that to raise)"""
    out = np.zeros(shape, dtype=np.asarray(nzval).dtype)
    out[np.asarray(rowval), np.repeat(np.arange(shape[1]), np.diff(colptr))] = nzval
    return out


def _host_stand_in(counts, test_name, device=0):
    """engine.normalize_counts on the host: preprocess.normalize + the CSC conversion of the device front-end -- an entry per present
    count, so the clr_nz value 0.0f of a sample's only OTU is a STORED zero.  Sparse tables only
    (what tests/test_meta_mask_cpu.py hands it; the traces give dense tables to preprocess.normalize)."""
    assert isinstance(counts, CSC) and counts.nzval.dtype == np.int32, "the OTU block must arrive as canonical Int32 counts"
    dense = _scatter(*counts)
    data, row_mask, col_mask = pre.normalize(dense, test_name)
    if test_name == "fz":
        return data, row_mask, col_mask
    data = data.astype(np.float32 if test_name == "fz_nz" else np.int32)
    present = dense[row_mask][:, col_mask] != 0 if test_name == "fz_nz" else data != 0
    cols, rows = np.nonzero(present.T)
    out = sp.csc_matrix(data.shape, dtype=data.dtype)
    out.indptr = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=data.shape[1])))).astype(np.int32)
    out.indices, out.data = rows.astype(np.int32), data[rows, cols]
    return out, row_mask, col_mask


def _recording_front_end(counts, test_name, **kw):
    """fw.api.normalize_counts for the traces: logs what it was handed; a dense table takes preprocess.normalize, a sparse one
    _host_stand_in."""
    _LOG.append(["normalize_counts", _rec(counts), test_name, _rec(kw)])
    return _host_stand_in(counts, test_name) if isinstance(counts, CSC) else pre.normalize(counts, test_name)


class RecordingEngine:
    """fw.api.Engine for the traces: logs every call, returns fixed edges, rejections and counters."""

    def __init__(self, *a, **kw):
        _LOG.append(["Engine", _rec(a), _rec(kw)])
        self.L = types.SimpleNamespace(fw_data_resident_bytes=None)

    def __getattr__(self, name):  # (whatever else a commit calls on the engine is logged by name and arguments)
        def call(*a, **kw):
            _LOG.append([name, _rec(a), _rec(kw)] if (a or kw) else [name])
        return call

    def lgl(self, **kw):
        _LOG.append(["lgl", _rec(kw)])
        return dict(edges=dict(EDGES), rejections=dict(REJECTIONS) if kw.get("track_rejections") else {})

    def counters(self):
        _LOG.append(["counters"])
        return {"cond_tests": 7}

    def data_resident_bytes(self):
        _LOG.append(["data_resident_bytes"])
        return 4096


def _values(a):
    if a.dtype.kind == "f":
        return [float(("%.9g" if a.dtype.itemsize <= 4 else "%.12g") % v) for v in a.ravel().tolist()]
    return a.ravel().tolist() if a.dtype.kind in "biu" else [repr(v) for v in a.ravel().tolist()]


def _rec(x):
    """anything a trace holds -> plain JSON data"""
    if isinstance(x, CSC):
        return {"CSC": [_rec(np.asarray(a)) for a in x[:3]], "shape": [int(v) for v in x[3]]}
    if sp.issparse(x):
        m = x if x.format == "csc" else x.tocsc()
        return {"sparse": x.format, "shape": list(x.shape), "arrays": [_rec(np.asarray(a)) for a in (m.indptr, m.indices, m.data)]}
    if isinstance(x, np.ndarray):
        return {"shape": list(x.shape), "dtype": str(x.dtype), "values": _values(x)}
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, dict):
        if all(isinstance(k, str) for k in x):
            return {k: _rec(v) for k, v in x.items()}
        return {"items": [[_rec(k), _rec(v)] for k, v in x.items()]}
    if isinstance(x, (list, tuple)):
        return [_rec(v) for v in x]
    return x if isinstance(x, (bool, int, float, str, type(None))) else repr(x)


def difference(got, exp, at="trace"):
    """The first place two traces differ, as a sentence, or None: floats to rtol=1e-6 / atol=1e-7, everything else exactly."""
    if type(got) is not type(exp):
        return "%s: %r is not %r" % (at, got, exp)
    if isinstance(got, float):
        return None if np.allclose(got, exp, rtol=1e-6, atol=1e-7, equal_nan=True) else "%s: %r is not %r" % (at, got, exp)
    if isinstance(got, dict):
        if list(got) != list(exp):
            return "%s: keys %s are not %s" % (at, list(got), list(exp))
        got, exp = list(got.values()), list(exp.values())
    if isinstance(got, list):
        if len(got) != len(exp):
            return "%s: %d entries, not %d: %r is not %r" % (at, len(got), len(exp), got, exp)
        return next((d for d in (difference(g, e, "%s[%d]" % (at, i)) for i, (g, e) in enumerate(zip(got, exp))) if d), None)
    return None if got == exp else "%s: %r is not %r" % (at, got, exp)


def pack(traces):
    """{case: trace} -> the golden file's content.  Only what repeats is folded, nothing is left out: every array is stored once, in
    "_arrays", and referred to as {"array": index}; parameters, counters and the keywords of Engine and of lgl are stored whole for the
    first case, in "_common", and as {"like": name, "but": {what differs}} wherever a case has the same keys in the same order."""
    first = next(t for t in traces.values() if "parameters" in t.get("result", ()))
    common = dict(parameters=first["result"]["parameters"], counters=first["result"]["counters"])
    common.update({c[0]: c[-1] for c in first["calls"] if c[0] in ("Engine", "lgl")})
    arrays, index = [], {}

    def fold(x, name=None):
        if isinstance(x, list):
            return [fold(v, x[0] if (i == len(x) - 1 and isinstance(x[0], str)) else None) for i, v in enumerate(x)]
        if not isinstance(x, dict):
            return x
        if "values" in x and "dtype" in x:
            return {"array": index.setdefault(json.dumps(x), len(index))}
        if name in common and list(x) == list(common[name]):
            return {"like": name, "but": {k: v for k, v in x.items() if v != common[name][k]}}
        return {k: fold(v, k) for k, v in x.items()}
    out = {"_common": common, "_arrays": arrays}
    out.update({k: fold(t) for k, t in traces.items()})
    arrays.extend(json.loads(s) for s in index)
    return out


def unpack(content):
    """what pack returned, or json.load gave back -> {case: trace}, every trace whole again"""
    common, arrays = content["_common"], content["_arrays"]

    def unfold(x):
        if isinstance(x, list):
            return [unfold(v) for v in x]
        if not isinstance(x, dict):
            return x
        if list(x) == ["array"]:
            return arrays[x["array"]]
        if list(x) == ["like", "but"]:
            return {k: x["but"].get(k, v) for k, v in common[x["like"]].items()}
        return {k: unfold(v) for k, v in x.items()}
    return {k: unfold(t) for k, t in content.items() if k not in ("_common", "_arrays")}


# ---- the tables -------------------------------------------------------------------------------------------------------------------
N = 6


def counts(p=8, salt=0, n=N):
    """n x p counts, about a third of them zero, no empty sample"""
    i, j = np.indices((n, p))
    x = (3 * i * i + 7 * j + i * j + 5 * salt) % 11
    x[x < 4] = 0
    x[:, 0] += 1 + i[:, 0] % 3
    return x.astype(np.int64)


def prepared(kind, p=8, salt=0):
    """stands for an already normalised matrix of `kind`"""
    x = counts(p, salt)
    return {"fz": (x - 3.0) / 4, "fz_nz": x / 4.0}[kind].astype(np.float32) if kind in ("fz", "fz_nz") else \
        ((x > 2) if kind == "mi" else np.minimum(x // 3, 2)).astype(np.int32)


ROWS = np.arange(N)
MASK = np.array([False, False, True, False, False, True, False, False])  # meta columns in the middle of the table
HEADER = ["otu%d" % j for j in range(8)]
HEADER_M = [("meta%d" if m else "otu%d") % j for j, m in enumerate(MASK)]
META = np.empty((N, 2), dtype=object)  # a numeric column and a string factor
META[:, 0], META[:, 1] = [0.5 + 0.25 * (i % 7) for i in ROWS], [["soil", "gut", "sea"][i % 3] for i in ROWS]


def masked(prepared_kind=None):
    """the 8-column table with a 0 / 1 column at 2 and a covariate at 5 (non-integral for a count table, a level for a prepared one)"""
    x = counts().astype(np.float64) if prepared_kind is None else prepared(prepared_kind)
    x = x.copy()
    x[:, 2] = ROWS % 2
    x[:, 5] = (0.5 + 0.25 * (ROWS % 7)) if prepared_kind is None else ROWS % 3
    return x


def with_empty_sample(p, salt):
    x = counts(p, salt)
    x[5] = 0
    return x


def _files(tmp):
    """the path-form inputs -> dict of paths"""
    f = {k: os.path.join(tmp, k) for k in ("main.tsv", "second.csv", "meta.tsv", "main_t.tsv", "table.txt")}
    fio.write_table(f["main.tsv"], counts(), HEADER)
    fio.write_table(f["second.csv"], counts(4, 2), ["its%d" % j for j in range(4)])
    fio.write_table(f["main_t.tsv"], counts().T, ["S%d" % (i + 1) for i in ROWS], row_ids=HEADER)
    with open(f["meta.tsv"], "w") as fh:
        fh.write("\tph\tsite\n" + "".join("S%d\t%r\t%s\n" % (i + 1, META[i, 0], META[i, 1]) for i in ROWS))
    open(f["table.txt"], "w").close()
    return f


# ---- the cases: name -> function of the path dict that makes ONE call ----------------------------------------------------------------
ln, nd, csc = fw.learn_network, fw.normalize_data, sp.csc_matrix
CASES = {}


def case(name, call):
    assert name not in CASES, name
    CASES[name] = call


def both(name, data, normalizing=True, **kw):
    """a learn_network case of kind fz_nz unless kw says otherwise and, when it normalises, its normalize_data counterpart"""
    kind = kw.pop("kind", "fz_nz")
    case("ln_" + name, lambda f: ln(data, **KINDS[kind], **kw))
    if normalizing:
        case("nd_" + name, lambda f: nd(data, test_name=kind, **kw))


for _k in KINDS:
    both("%s_dense_host" % _k, counts(), kind=_k, device_normalize=False)
    both("%s_dense_stand_in" % _k, counts(), kind=_k)
    both("%s_csc" % _k, csc(counts()), kind=_k)
    both("%s_dense_prepared" % _k, prepared(_k), False, kind=_k, normalize=False)
    both("%s_csc_prepared" % _k, csc(prepared(_k)), False, kind=_k, normalize=False)  # (fz: a refusal)
for _k in ("fz_nz", "mi"):
    # meta_data: a numeric column and a string factor
    both("%s_meta_data_onehot" % _k, counts(), kind=_k, meta_data=META, meta_header=["ph", "site"], device_normalize=False)
    both("%s_meta_data_no_onehot" % _k, counts(), kind=_k, meta_data=META, meta_header=["ph", "site"], make_onehot=False,
         device_normalize=False)
    # meta_mask in the middle of the table
    both("%s_mask_dense" % _k, masked(), kind=_k, meta_mask=MASK, header=HEADER_M, device_normalize=False)
    both("%s_mask_csc" % _k, csc(masked()), kind=_k, meta_mask=MASK)
both("meta_data_stand_in", counts(), meta_data=META[:, :1].astype(np.float64), header=HEADER)
both("meta_data_numbers_no_onehot", counts(), kind="mi_nz", meta_data=META[:, :1].astype(np.float64), make_onehot=False, device_normalize=False)
both("mask_dense_stand_in_no_header", masked(), meta_mask=MASK)
both("mask_csc_header", csc(masked()), kind="mi_nz", meta_mask=[int(m) for m in MASK], header=HEADER_M)
both("mask_all_false_dense", counts(), meta_mask=np.zeros(8, bool), device_normalize=False)
both("mask_all_false_csc", sp.csr_matrix(counts()), kind="mi", meta_mask=np.zeros(8, bool), header=HEADER)
for _k in ("fz_nz", "mi_nz"):
    both("mask_dense_prepared_%s" % _k, masked(_k), False, kind=_k, normalize=False, meta_mask=MASK, header=HEADER_M)
    both("mask_csc_prepared_%s" % _k, csc(masked(_k)), False, kind=_k, normalize=False, meta_mask=MASK)
both("mask_all_false_prepared", prepared("mi"), False, kind="mi", normalize=False, meta_mask=[0] * 8)

# extra_data
_E1, _E2 = counts(4, 2), counts(3, 5)
both("extra_no_header", counts(), extra_data=[(_E1, None)], device_normalize=False)
both("extra_named", counts(), kind="mi_nz", extra_data=[(_E1, ["its%d" % j for j in range(4)])], header=HEADER)
both("extra_two", counts(), kind="fz", extra_data=[(_E1, None), (_E2.astype(np.float64) / 2, ["b0", "b1", "b2"])])  # (host: not integral)
both("extra_two_no_headers", counts(), kind="mi", extra_data=[(_E1, None), (_E2, None)])
both("extra_under_mask", masked(), kind="mi_nz", meta_mask=MASK, extra_data=[(_E1, None), (_E2, ["b0", "b1", "b2"]), (_E1, None)],
     device_normalize=False)
both("extra_under_mask_csc", csc(masked()), meta_mask=MASK, header=HEADER_M, extra_data=[(csc(_E1), None)])
both("extra_csc", csc(counts()), kind="mi_nz", extra_data=[(sp.coo_matrix(_E1), None), (csc(_E2), ["b0", "b1", "b2"])])
both("extra_dropped_sample", counts(), extra_data=[(with_empty_sample(4, 2), None)], device_normalize=False)
both("extra_dropped_sample_csc", csc(counts()), kind="mi_nz", extra_data=[(csc(with_empty_sample(4, 2)), None)])
both("extra_prepared", prepared("fz_nz"), False, normalize=False, extra_data=[(prepared("fz_nz", 4, 2), None), (prepared("fz_nz", 3, 5), None)])
both("extra_prepared_mask", masked("mi_nz"), False, kind="mi_nz", normalize=False, meta_mask=MASK, header=HEADER_M,
     extra_data=[(prepared("mi_nz", 4, 2), None)])
both("extra_prepared_csc_mask", csc(masked("fz_nz")), False, normalize=False, meta_mask=MASK,
     extra_data=[(csc(prepared("fz_nz", 4, 2)), ["its%d" % j for j in range(4)])])
both("extra_empty_list", counts(), extra_data=[], device_normalize=False)
both("header_too_short_no_mask", counts(), header=HEADER[:5], device_normalize=False)  # (learn_network: zip truncates)
both("header_too_long_no_mask_prepared", prepared("fz"), False, kind="fz", normalize=False, header=HEADER + ["more"])

# the path form
case("ln_path_one_tsv", lambda f: ln(f["main.tsv"], **KINDS["fz_nz"], device_normalize=False))
case("ln_path_pathlike", lambda f: ln(pathlib.Path(f["main.tsv"]), **KINDS["mi"]))
case("ln_path_two_and_meta", lambda f: ln([f["main.tsv"], f["second.csv"]], f["meta.tsv"], **KINDS["mi_nz"], device_normalize=False))
case("ln_path_transposed", lambda f: ln(f["main_t.tsv"], transposed=True, **KINDS["fz"]))
case("ln_path_list_with_extra_data", lambda f: ln([f["main.tsv"], f["second.csv"]], **KINDS["fz_nz"], extra_data=[(_E2, None)]))
case("ln_path_one_with_extra_data", lambda f: ln((f["main.tsv"],), **KINDS["fz_nz"], extra_data=[(_E2, ["b0", "b1", "b2"])], normalize=False))
case("ln_path_unreadable_format", lambda f: ln(f["table.txt"]))

# engine options
both("csc_resident", csc(counts()), False, csc_resident=True)
both("csc_resident_truthy_under_mask", csc(masked()), False, csc_resident=1, meta_mask=MASK)
both("prec64_fz", counts(), kind="fz", prec=64)
both("prec64_fz_prepared", prepared("fz").astype(np.float64), False, kind="fz", prec=64, normalize=False)
both("prec64_mi", counts(), kind="mi", prec=64)
both("prec64_fz_nz_host", counts(), prec=64, device_normalize=False)
both("no_dense_cor_default_pcor", counts(), False, kind="fz", dense_cor=False)  # (the warning)
both("no_dense_cor_no_pcor", counts(), False, kind="fz", dense_cor=False, recursive_pcor=False)
both("no_dense_cor_mi", counts(), False, kind="mi", dense_cor=False)
both("no_dense_cor_fz_nz_no_pcor", counts(), False, dense_cor=False, recursive_pcor=False)
both("no_pcor_fz", counts(), False, kind="fz", recursive_pcor=False)
for _r in (None, 0, 1, 3, 6, 64):
    both("round_size_%s" % _r, prepared("fz", 6), False, kind="fz", normalize=False, round_size=_r)
both("no_feed_forward", counts(), False, kind="mi_nz", feed_forward=False, round_size=3)
both("exact_elim_tracked", counts(), False, kind="fz", fast_elim=False, no_red_tests=False, track_rejections=True)
both("numbers", counts(), False, kind="mi", max_k=1, alpha=0.05, hps=3, FDR=False, n_obs_min=20, max_tests=1000, device=3)
both("world_of_none", counts(), False, distributed=False, track_rejections=1, fast_elim=0)

# normalize_data on its own
case("nd_bad_test_name", lambda f: nd(counts(), test_name="fz64"))
case("nd_bad_prec", lambda f: nd(counts(), prec=16))
case("nd_bad_test_name_and_prec", lambda f: nd(counts(), test_name="clr", prec=16))
case("nd_header_too_long", lambda f: nd(counts(), header=HEADER + ["more"]))
case("nd_csc_tuple", lambda f: nd(CSC(*(lambda m: (m.indptr, m.indices, m.data, m.shape))(csc(counts()))), test_name="mi_nz"))
case("nd_plain_tuple_is_dense", lambda f: nd(tuple(map(tuple, counts())), test_name="mi", device_normalize=False))
case("nd_csc_tuple_under_mask", lambda f: nd(CSC(*(lambda m: (m.indptr, m.indices, m.data, m.shape))(csc(masked()))), test_name="fz_nz",
                                             meta_mask=MASK, extra_data=[(csc(_E1), None)]))
case("nd_header_too_short_under_mask_and_bad_extra", lambda f: nd(masked(), header=HEADER[:5], meta_mask=MASK, extra_data=[(_E1[:-1], None)]))
case("nd_header_too_short_and_bad_extra", lambda f: nd(counts(), header=HEADER[:5], extra_data=[(_E1[:-1], None)]))
case("ln_csc_tuple", lambda f: ln(CSC(*(lambda m: (m.indptr, m.indices, m.data, m.shape))(csc(counts()))), **KINDS["mi_nz"]))

# single refusals: every raise statement of api.py
_NOT_COUNTS, _STRINGS = csc(counts() + 0.5), masked().astype(object)
_STRINGS[:, 5] = ["x"] * N
_NAN = masked()
_NAN[3, 5] = np.nan
case("ln_unsupported_option", lambda f: ln(counts(), verbose=True, parallel="single"))
case("ln_bad_prec", lambda f: ln(counts(), prec=16))
case("ln_meta_data_path_with_array", lambda f: ln(counts(), "meta.tsv"))
case("ln_transposed_with_array", lambda f: ln(counts(), transposed=True))
case("ln_meta_data_path_no_path", lambda f: ln(f["main.tsv"], 3))
case("ln_path_with_header", lambda f: ln(f["main.tsv"], header=HEADER))
case("ln_path_with_meta_data", lambda f: ln(f["main.tsv"], meta_data=META))
case("ln_path_with_meta_header", lambda f: ln([f["main.tsv"]], meta_header=["ph"]))
case("ln_path_with_meta_mask", lambda f: ln(f["main.tsv"], meta_mask=MASK))
case("ln_distributed_no_group", lambda f: ln(counts(), distributed=True))
both("sparse_host_front_end", csc(counts()), device_normalize=False)
both("sparse_prec64", csc(counts()), prec=64)
both("sparse_meta_data", csc(counts()), meta_data=META)
both("sparse_not_counts", _NOT_COUNTS)
both("sparse_no_levels", _NOT_COUNTS, False, kind="mi_nz", normalize=False)
both("mask_with_meta_data", masked(), meta_mask=MASK, meta_data=META)
both("mask_on_a_vector", counts()[:, 0], meta_mask=[True])
both("mask_too_short", masked(), meta_mask=MASK[:-1])
both("mask_two_dimensional", masked(), meta_mask=np.stack([MASK, MASK]))
both("mask_no_booleans", masked(), meta_mask=np.where(MASK, 2, 0))
both("mask_strings", masked(), meta_mask=["yes" if m else "no" for m in MASK])
both("mask_every_column", masked(), meta_mask=np.ones(8, bool))
both("mask_marks_strings", _STRINGS, meta_mask=MASK)
both("mask_marks_nan", _NAN, meta_mask=MASK)
both("mask_marks_nan_csc", csc(_NAN), meta_mask=MASK)
both("mask_marks_strings_prepared", _STRINGS, False, normalize=False, meta_mask=MASK)
both("mask_marks_nan_csc_prepared", csc(_NAN), False, normalize=False, meta_mask=MASK)
both("mask_csc_otu_block_not_counts", csc(masked()), kind="mi", meta_mask=[False, False, True] + [False] * 5)
both("extra_not_a_list", counts(), extra_data=_E1)
both("extra_no_pair", counts(), extra_data=[(_E1, None), _E2])
both("extra_table_of_strings", counts(), extra_data=[(np.array([["a"]]), None)])
both("extra_table_a_vector", counts(), extra_data=[(_E1[:, 0], None)])
both("extra_header_a_string", counts(), extra_data=[(_E1, "its")])
both("extra_header_a_number", counts(), extra_data=[(_E1, 4)])
both("extra_mix_dense_main", counts(), extra_data=[(csc(_E1), None)])
both("extra_mix_sparse_main", csc(counts()), extra_data=[(_E1, None)])
both("extra_other_rows", counts(), extra_data=[(_E1, None), (_E2[:-1], None)])
both("extra_header_length", counts(), extra_data=[(_E1, ["a", "b"])])
both("extra_csc_not_counts", csc(counts()), extra_data=[(_NOT_COUNTS, None)])
case("ln_csc_resident_other_mode", lambda f: ln(csc(counts()), **KINDS["mi_nz"], csc_resident=True))
case("ln_csc_resident_dense", lambda f: ln(counts(), **KINDS["fz_nz"], csc_resident=True))
case("ln_csc_resident_no_pcor", lambda f: ln(csc(counts()), **KINDS["fz_nz"], csc_resident=True, recursive_pcor=False))
case("ln_prec64_no_pcor", lambda f: ln(counts(), prec=64, recursive_pcor=False))
case("ln_prec64_no_dense_cor", lambda f: ln(counts(), prec=64, dense_cor=False))
case("ln_mask_header_length", lambda f: ln(masked(), meta_mask=MASK, header=HEADER[:5]))
case("ln_meta_data_prepared", lambda f: ln(prepared("fz"), normalize=False, meta_data=META))

# double refusals: the order is part of the contract
case("two_unsupported_and_bad_prec", lambda f: ln(counts(), prec=16, verbose=True))
case("two_bad_prec_and_meta_data_path", lambda f: ln(counts(), "meta.tsv", prec=128))
case("two_meta_data_path_and_transposed", lambda f: ln(counts(), "meta.tsv", transposed=True))
case("two_path_header_and_meta_mask", lambda f: ln(f["main.tsv"], header=HEADER, meta_mask=MASK))
case("two_path_meta_data_path_and_header", lambda f: ln(f["main.tsv"], 3, header=HEADER))
case("two_path_meta_mask_and_unreadable", lambda f: ln(f["table.txt"], meta_mask=MASK))
case("two_distributed_and_csc_resident", lambda f: ln(counts(), distributed=True, csc_resident=True))
case("two_csc_resident_mode_and_prec64_no_pcor", lambda f: ln(csc(counts()), csc_resident=True, prec=64, recursive_pcor=False))
case("two_csc_resident_mode_and_dense", lambda f: ln(counts(), **KINDS["mi"], csc_resident=True))
case("two_csc_resident_dense_and_no_pcor", lambda f: ln(counts(), **KINDS["fz_nz"], csc_resident=True, recursive_pcor=False))
case("two_csc_resident_no_pcor_and_sparse_host", lambda f: ln(csc(counts()), **KINDS["fz_nz"], csc_resident=True, recursive_pcor=False,
                                                              device_normalize=False))
case("two_prec64_no_dense_cor_and_mask", lambda f: ln(masked(), prec=64, dense_cor=False, meta_mask=MASK[:-1]))
case("two_warning_then_sparse_refusal", lambda f: ln(csc(counts()), dense_cor=False, device_normalize=False))  # (the warning, then the refusal)
both("two_sparse_host_and_mask_length", csc(masked()), device_normalize=False, meta_mask=MASK[:-1])
both("two_mask_meta_data_on_sparse", csc(masked()), meta_mask=MASK, meta_data=META)
both("two_sparse_prec64_and_meta_data", csc(counts()), prec=64, meta_data=META)
both("two_sparse_fz_prepared_and_mask_header", csc(prepared("fz")), False, kind="fz", normalize=False, meta_mask=MASK, header=HEADER[:5])
both("two_mask_header_and_extra_rows", masked(), meta_mask=MASK, header=HEADER[:5], extra_data=[(_E1[:-1], None)])
both("two_mask_header_and_marked_nan", _NAN, meta_mask=MASK, header=HEADER[:5])
both("two_sparse_not_counts_and_extra", _NOT_COUNTS, extra_data=_E1)
both("two_marked_nan_and_extra_prepared", _NAN, False, normalize=False, meta_mask=MASK, extra_data=[_E1])
both("two_marked_nan_and_extra", _NAN, meta_mask=MASK, extra_data=[_E1])
both("two_meta_data_prepared_and_extra", prepared("fz"), False, kind="fz", normalize=False, meta_data=META, extra_data=[(_E1,)])
both("two_extra_rows_then_pair", counts(), extra_data=[(_E1[:-1], None), _E2])
both("two_extra_mix_and_rows", counts(), extra_data=[(csc(_E1[:-1]), None)])


def run_case(name, files):
    """One case -> its trace, as plain JSON data (what json.load gives back)."""
    saved = fw.api.Engine, fw.api.normalize_counts
    fw.api.Engine, fw.api.normalize_counts = RecordingEngine, _recording_front_end
    del _LOG[:]
    trace = {}
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            try:
                r = CASES[name](files)
            except Exception as e:  # noqa: BLE001 -- the type and the message ARE the trace
                trace["raised"] = [type(e).__name__, str(e)]
            else:
                r = dict(r)
                if "counters" in r:
                    r["counters"] = dict(r["counters"])
                    t = r["counters"].pop("t_normalize_s")
                    assert isinstance(t, float) and t >= 0, t
                trace["result"] = _rec(r)
        here = os.path.splitext(os.path.abspath(__file__))[0]
        trace["warnings"] = [[w.category.__name__, str(w.message), os.path.splitext(os.path.abspath(w.filename))[0] == here]
                             for w in caught if "flashweave" in w.filename or os.path.splitext(os.path.abspath(w.filename))[0] == here]
        trace["calls"] = list(_LOG)
    finally:
        fw.api.Engine, fw.api.normalize_counts = saved
    return json.loads(json.dumps(trace))


def run_all():
    with tempfile.TemporaryDirectory() as tmp:
        files = _files(tmp)
        return {name: run_case(name, files) for name in CASES}


def load_golden():
    with open(GOLDEN_FILE) as fh:
        return unpack(json.load(fh))


if __name__ == "__main__":
    traces = run_all()
    if "--write" in sys.argv[1:]:
        def line(v):
            return json.dumps(v, separators=(",", ":"))
        content = pack(traces)
        assert unpack(json.loads(json.dumps(content))) == traces
        with open(GOLDEN_FILE, "w") as fh:  # a case, and an array, per line
            fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), "[\n" + ",\n".join(map(line, v)) + "\n]" if k == "_arrays" else line(v))
                                        for k, v in content.items()) + "\n}\n")
        print("wrote %d cases, %d bytes -> %s" % (len(traces), os.path.getsize(GOLDEN_FILE), GOLDEN_FILE))
    else:
        for k, v in traces.items():
            print(k, "->", v.get("raised") or "ok", v["warnings"] or "")
