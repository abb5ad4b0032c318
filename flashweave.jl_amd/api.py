"""`learn_network`: the reference's user entry point (src/learning.jl:466-598) for the modes this engine covers, as a thin
composition of the normalisation front-end, the device engine and the host driver.  Keyword names and defaults
follow the reference; unsupported options raise instead of being silently ignored."""
import os
import time
import warnings
from collections import namedtuple

import numpy as np

from . import io as fio
from . import preprocess as pre
from .engine import (CSC, Engine, abundance_defect, as_csc, is_device_tensor, is_sparse, is_sparse_csc_tensor, normalize_abundances,
                     normalize_counts, rejections_dict, tss_range_defect)


class FWResult(dict):
    """Edge list + bookkeeping (the reference's FWResult, src/types.jl:172-200, reduced to plain data)."""

    def save(self, path):
        """save_network (src/io.jl:300-336): .edgelist or .gml by extension."""
        fio.save_network(path, self["edges"], self["variable_ids"], self["meta_variable_mask"])

    def save_rejections(self, path, digits=5):
        """save_rejections (src/io.jl:296-318)."""
        fio.save_rejections(path, self, digits=digits)


def default_round_size(p):
    """Targets per feed-forward round when the caller does not choose.

    p <= 512: 1 -- the reference's deterministic `single_il` schedule (interleaved.jl:62-183; what its golden networks were
    generated with), so the default output of a small problem IS the reference's network.  Larger problems: rounds of
    min(1024 * ceil(p / 10240), max(64, ceil(p / 8))) targets -- eight to ten rounds per pass, so that whitelists exist at every
    size (one round would silently turn feed_forward off), each of them on the device (fz: device-resident rounds, discrete: one
    persistent launch).  At the benchmark sizes this is the schedule bench.py reports (cfg3 1024, cfg4 5120, cfg5 10 240).  The result records which schedule ran
    (`parameters["schedule"]`): rounds deviate from single_il in when the whitelists refresh, not in the tests themselves."""
    if p <= 512:
        return 1
    return min(1024 * ((p + 10239) // 10240), max(64, (p + 7) // 8))


def _integral(a):
    """Count table the device front-end accepts: integral values in 0 .. 2^31 - 1 (fw_normalize_counts takes Int32); anything else
    -- relative abundances, negative entries, counts beyond Int32 -- goes to the host front-end (preprocess.py)."""
    if is_device_tensor("_integral", a):
        return _integral_tensor(a)
    if not a.size:
        return False
    if np.issubdtype(a.dtype, np.integer):
        return bool(a.min() >= 0 and a.max() < 2**31)
    return bool(np.issubdtype(a.dtype, np.floating) and np.all(np.isfinite(a)) and np.all(a == np.floor(a)) and
                a.max() < 2**31 and a.min() >= 0)



def _integral_tensor(t):
    """_integral for a table in GPU memory, in torch ops on the device (booleans count as 0 / 1)"""
    import torch
    t = t.values() if is_sparse_csc_tensor(t) else t  # (a sparse CSC tensor: its stored values; the absent cells are zeros)
    if not t.numel() or t.dtype.is_complex:
        return False
    if t.dtype.is_floating_point and not (bool(torch.isfinite(t).all()) and bool((t == torch.floor(t)).all())):
        return False
    return t.dtype == torch.bool or bool(float(t.min()) >= 0 and float(t.max()) < 2**31)


def _tensor_refusals(who, t, device, normalize, abundances, meta_data=None, meta_mask=None, extra_data=None, prec=32, device_normalize=True,
                     distributed=False, csc_resident=False):
    """What a table in GPU memory (a torch tensor, engine.is_device_tensor) is not served with: each would need the table's bytes on
    the host, and copying silently would defeat the point.  Every refusal names its option and the way out (tensor.cpu()), before any
    library call; the last one looks at the values, with torch ops on the device.  A sparse CSC tensor is the sparse table of this
    path and gets the same refusals but csc_resident=True (served, for fz_nz); every other sparse layout is refused."""
    import torch

    def no(option, why):
        raise ValueError("%s: %s with a table in GPU memory is not supported: %s; pass tensor.cpu() instead" % (who, option, why))
    if t.layout not in (torch.strided, torch.sparse_csc):
        raise ValueError("%s: a sparse torch tensor is not supported: scipy.sparse is the sparse interface; build a scipy matrix from "
                         "tensor.cpu() instead (or pass tensor.to_dense()); of the sparse layouts only tensor.to_sparse_csc() is taken" % who)
    numeric = t.dtype.is_floating_point or t.dtype in (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)
    if t.dim() != 2 or not numeric:
        raise ValueError("%s: a device tensor must be a 2-D samples x variables table of a numeric dtype (got %d dimensions, %s); "
                         "pass tensor.cpu() instead if it is something else" % (who, t.dim(), t.dtype))
    if meta_data is not None:
        no("meta_data", "meta variables are prepared on the host")
    if meta_mask is not None:
        no("meta_mask", "meta variables are prepared on the host")
    if extra_data is not None:
        no("extra_data", "several tables are combined on the host")
    if prec == 64:
        no("prec=64", "the Float64 mode uploads from the host")
    if not device_normalize:
        no("device_normalize=False", "the host front-end reads host memory")
    if distributed:
        no("distributed=True", "the digest the ranks compare needs the table's bytes on the host")
    if csc_resident and t.layout == torch.strided:
        no("csc_resident=True", "the CSC-resident layout is built from a scipy.sparse matrix")
    if t.device.index != device:
        raise ValueError("%s: device=%d while the tensor lives on %s: pass the device the table is on, or tensor.cpu() instead"
                         % (who, device, t.device))
    if normalize and not abundances and not _integral_tensor(t):
        raise ValueError("%s: the tensor does not hold integral counts in 0 .. 2^31 - 1 and abundances=True is not given: pass "
                         "abundances=True for a real-valued table in GPU memory, or tensor.cpu() instead for the host front-end" % who)


_TEST_NAMES = ("fz", "fz_nz", "mi", "mi_nz")
# normalize_data's norm_mode (preprocessing.jl:660-684) -> the test_name it stands for (four aliases) or goes with (the two TSS modes,
# preprocess.TSS_NORMS: no test_name selects them)
_NORM_MODES = {"clr-adapt": "fz", "clr-nonzero": "fz_nz", "clr-nonzero-binned": "mi_nz", "pres-abs": "mi", **pre.TSS_NORMS}
# learn_network's keywords by where they go.  All of them -- the caller's values, before anything is resolved -- go into the digest
# of a distributed run; parameters= reports _REPORTED, the Engine takes _ENGINE_KEYS and lgl _LGL_KEYS, each with the resolved values
# (test_name, round_size, recursive_pcor, dense_cor, csc_resident, prec = the engine's element type) laid over the caller's.
_REPORTED = ("sensitive", "heterogeneous", "max_k", "alpha", "feed_forward", "test_name", "round_size", "recursive_pcor", "dense_cor",
             "fast_elim", "no_red_tests", "track_rejections", "prec", "csc_resident")
_ENGINE_KEYS = ("max_k", "alpha", "hps", "n_obs_min", "max_tests", "FDR", "device", "recursive_pcor", "dense_cor", "prec")
_LGL_KEYS = ("feed_forward", "round_size", "fast_elim", "no_red_tests", "track_rejections")
_NEIGHBORS_KEYS = ("fast_elim", "no_red_tests", "track_rejections")  # Engine.neighbors (learn_neighbors: no schedule to choose)


def _is_path(x):
    return isinstance(x, (str, os.PathLike))


def _any_sparse(x):
    """A sparse table in any of its forms: a scipy.sparse matrix / array, or the canonical triple as_csc returned."""
    return is_sparse(x) or isinstance(x, CSC)


def _default_header(cols, start=0):
    """X(start + 1) .. X(start + cols): the names of columns that came without any, numbered on from `start` columns before them."""
    return ["X%d" % (start + j + 1) for j in range(cols)]


def _path_form(data, meta_data_path, transposed, header, meta_data, meta_header, meta_mask, extra_data, who="learn_network"):
    """learn_network(data_path | all_data_paths, meta_data_path) (learning.jl:354-401) -> (data, header, meta_data, meta_header,
    extra_data) as arrays: the first path is the main table, the others become extra_data with their file headers, ahead of the
    caller's; only the main table has meta data.  io.load_data decides what is readable.  Arrays pass through as they are."""
    paths = [data] if _is_path(data) else list(data) if (isinstance(data, (list, tuple)) and len(data) and all(_is_path(q) for q in data)) else None
    if paths is None:
        if meta_data_path is not None:
            raise ValueError("%s: meta_data_path goes with a data path (%s(data_path, meta_data_path)); with an "
                             "array pass meta_data" % (who, who))
        if transposed:
            raise ValueError("%s: transposed=True is served for the path form; pass the transposed array" % who)
        return data, header, meta_data, meta_header, extra_data
    if not (meta_data_path is None or _is_path(meta_data_path)):
        raise TypeError("%s: meta_data_path must be a path, got %s (options are keywords)" % (who, type(meta_data_path).__name__))
    if header is not None or meta_data is not None or meta_header is not None:
        raise ValueError("%s: header, meta_data and meta_header come from the files in the path form" % who)
    if meta_mask is not None:
        raise ValueError("%s: meta_mask goes with an array or a sparse matrix; in the path form the meta variables come "
                         "from meta_data_path" % who)
    meta_path = None if meta_data_path is None else os.fspath(meta_data_path)
    data, header, meta_data, meta_header = fio.load_data(os.fspath(paths[0]), meta_path, transposed=transposed)
    from_files = [fio.load_data(os.fspath(q), None, transposed=transposed)[:2] for q in paths[1:]]
    return data, header, meta_data, meta_header, (from_files + list(extra_data or []) if (from_files or extra_data is not None) else None)


def _sparse_refusals(who, test_name, normalize, prec, device_normalize, meta_data):
    """What a sparse table is not served with: each would need the dense matrix, and densifying silently would defeat the point."""
    if not device_normalize:
        raise ValueError("%s: sparse data with device_normalize=False is not supported: the host front-end "
                         "(preprocess.py) is dense; pass data.toarray() or leave device_normalize=True" % who)
    if prec == 64:
        raise ValueError("%s: sparse data with prec=64 is not supported: the Float64 path takes a dense matrix" % who)
    if meta_data is not None:
        raise ValueError("%s: sparse data with meta_data is not supported: append the prepared meta columns to "
                         "`data` yourself (preprocess.normalize_with_meta), or pass the meta columns inside `data` and mark them "
                         "with meta_mask" % who)
    if test_name == "fz" and not normalize:
        raise ValueError("%s: sparse data with sensitive=True, heterogeneous=False, normalize=False is not supported: "
                         "the plain fz test needs the dense matrix, pass one" % who)


def _canonical_csc(who, data, test_name, normalize, abundances=False):
    if abundances and normalize:  # real values: nothing is checked as a count (the values themselves: _abundance_refusals)
        try:
            return as_csc(data, np.float64)
        except ValueError as e:
            raise ValueError("%s: abundances=True: sparse data needs real values (%s)" % (who, e)) from None
    try:
        return as_csc(data, np.int32 if (normalize or test_name in ("mi", "mi_nz")) else np.float32)
    except ValueError as e:
        raise ValueError("%s: sparse data with normalize=%s needs %s (%s)"
                         % (who, normalize, "integer counts in 0 .. 2^31 - 1: the device front-end takes nothing else" if normalize
                            else "integer levels", e)) from None


def _shape(t):
    return tuple(t[3]) if isinstance(t, CSC) else tuple(t.shape)


def _meta_mask_vector(who, meta_mask, meta_data, data):
    """learn_network's / normalize_data's meta_mask against the table (an array or a sparse table) -> a bool vector, or None when no
    column is marked (an all-False mask is no mask)."""
    if meta_mask is None:
        return None
    if meta_data is not None:
        raise ValueError("%s: meta_mask together with meta_data is not supported: meta variables come inside `data` under a "
                         "meta_mask or as a table of their own, not both" % who)
    if len(_shape(data)) != 2:
        raise ValueError("%s: meta_mask needs a samples x variables matrix, got %d dimensions" % (who, len(_shape(data))))
    m, cols = np.asarray(meta_mask), _shape(data)[1]
    if m.ndim != 1 or m.size != cols:
        raise ValueError("%s: meta_mask has %s for the %d columns of data: one entry per column, the meta columns included"
                         % (who, "%d entries" % m.size if m.ndim == 1 else "%d dimensions" % m.ndim, cols))
    if m.dtype.kind not in "biuf" or not np.all((m == 0) | (m == 1)):
        raise ValueError("%s: meta_mask must hold booleans (or 0 / 1), True marking a meta variable" % who)
    m = m.astype(bool)
    if m.all():
        raise ValueError("%s: meta_mask marks every column: no OTU column is left to normalise" % who)
    return m if m.any() else None


def _finite_meta(who, values):
    if values.dtype.kind not in "biuf":
        raise ValueError("%s: the columns meta_mask marks must be numbers (got %s); string factors go through meta_data" % (who, values.dtype))
    if values.dtype.kind == "f" and not np.all(np.isfinite(values)):
        raise ValueError("%s: a column meta_mask marks holds a non-finite value (NaN or Inf)" % who)


def _csc_arrays(data):
    """A sparse table as it comes -> (colptr, rowval, nzval, (n, p)) without the count check (values, duplicates and order as stored)."""
    if isinstance(data, (CSC, tuple)):
        return data[0], data[1], data[2], tuple(int(v) for v in data[3])
    import scipy.sparse as sp
    m = sp.csc_matrix(data)
    return m.indptr, m.indices, m.data, tuple(int(v) for v in m.shape)


def _split_meta(who, data, mask, header, test_name, abundances=False):
    """The table of a normalising run under its meta_mask -> (OTU block, its header, meta block, its header), before anything is checked
    as a count: the unmarked columns are the count table (a sparse one canonical, _canonical_csc), the marked ones a dense Float64
    samples x meta-variables matrix (a continuous covariate is not a count).  A sparse table is split on its CSC arrays, O(nnz); only
    the few meta columns are densified."""
    otu_header, meta_header = [h for h, m in zip(header, mask) if not m], [h for h, m in zip(header, mask) if m]
    if not _any_sparse(data):
        meta = data[:, mask]
        _finite_meta(who, meta)
        return data[:, ~mask], otu_header, meta.astype(np.float64), meta_header
    colptr, rowval, nzval, (n, p) = _csc_arrays(data)
    q = int(mask.sum())
    otu = _canonical_csc(who, pre._csc_take_cols(colptr, rowval, nzval, np.nonzero(~mask)[0]) + ((n, p - q),), test_name, True, abundances)
    meta = as_csc(pre._csc_take_cols(colptr, rowval, nzval, np.nonzero(mask)[0]) + ((n, q),), np.float64)
    _finite_meta(who, meta.nzval)
    return otu, otu_header, pre._csc_to_dense(meta.colptr, meta.rowval, meta.nzval, n), meta_header


def _extra_tables(who, data, extra_data, test_name, normalize, n_named=None, abundances=False):
    """Checks learn_network's / normalize_data's extra_data against the main table (an array or what as_csc returned) before anything
    reaches a device -> [(table, header)] in the caller's order, sparse tables canonical.  A missing header is numbered on from the
    main table's columns (n_named when the meta columns have been split off `data` already), as the reference does
    (learning.jl:506-520)."""
    if extra_data is None:
        return []
    sparse, (n, cols) = isinstance(data, CSC), _shape(data)
    n_named = cols if n_named is None else n_named
    if not isinstance(extra_data, (list, tuple)):
        raise ValueError("%s: extra_data must be a list of (table, header) pairs, got %s" % (who, type(extra_data).__name__))
    out = []
    for i, entry in enumerate(extra_data):
        if not (isinstance(entry, (list, tuple)) and len(entry) == 2):
            raise ValueError("%s: extra_data[%d] is not a (table, header) pair" % (who, i))
        tab, hdr = entry
        if not _any_sparse(tab):
            tab = np.asarray(tab)
            if tab.ndim != 2 or tab.dtype.kind not in "biuf":
                raise ValueError("%s: extra_data[%d] is not a (table, header) pair: the table must be a samples x OTUs matrix of "
                                 "numbers" % (who, i))
        if hdr is not None and (isinstance(hdr, (str, bytes)) or not hasattr(hdr, "__len__")):
            raise ValueError("%s: extra_data[%d] is not a (table, header) pair: the header must be a list of names or None" % (who, i))
        if _any_sparse(tab) != sparse:
            raise ValueError("%s: extra_data[%d] is %s while data is %s: a mix of sparse and dense tables is not supported, pass all "
                             "of them in one form" % (who, i, "dense" if sparse else "sparse", "sparse" if sparse else "dense"))
        rows, cols = _shape(tab)
        if rows != n:
            raise ValueError("%s: extra_data[%d] has %d rows, data has %d: every table holds the same samples in the same order"
                             % (who, i, rows, n))
        if hdr is None:
            hdr = _default_header(cols, n_named)
            n_named += cols
        elif len(hdr) != cols:
            raise ValueError("%s: extra_data[%d] has a header of %d names for %d columns" % (who, i, len(hdr), cols))
        out.append((tab, [str(h) for h in hdr]))
    return [(_canonical_csc(who, t, test_name, normalize, abundances), h) for t, h in out] if sparse else out


def _abundance_refusals(who, data, extra):
    """abundances=True: every table of real values (the OTU block where a meta_mask split the table) holds finite values >= 0."""
    for name, tab in [("data", data)] + [("extra_data[%d]" % i, t) for i, (t, _) in enumerate(extra)]:
        defect = abundance_defect(tab.nzval if isinstance(tab, CSC) else tab.values() if is_sparse_csc_tensor(tab) else tab)
        if defect:
            raise ValueError("%s: abundances=True: %s holds %s; abundances are finite and >= 0" % (who, name, defect))


def _normalize_tables(data, header, extra, test_name, meta_data, meta_header, make_onehot, prec, device_normalize, device, abundances=False,
                      tss=None, bins=None):
    """Every table through ONE front-end -- the device one when all of them are count tables it takes (sparse, or _integral) and
    prec == 32 and device_normalize, else the host one -- each on its own (its own row sums, geometric means, pseudo-counts and
    filters), then preprocess.combine_data.  abundances: the tables are declared real-valued, _integral is not asked and the device
    front-end is the Float64 one (engine.normalize_abundances).  tss: one of preprocess.TSS_NORMS, handed to whichever front-end runs
    as norm= (test_name is then the one the norm goes with); None hands every front-end what it was always handed.  bins: those of
    n_bins, rank_method and disc_method that are away from their defaults (preprocess.bins_kw), handed to whichever front-end runs as
    keywords, for every table alike; None or {} adds no keyword.  The meta variables never take them (2 bins, preprocessing.jl:531-533).
    -> (dict(data, header, meta_mask, row_mask), on_device)"""
    on_device = bool(device_normalize and prec == 32 and
                     (abundances or all(isinstance(t, CSC) or _integral(t) for t in [data] + [t for t, _ in extra])))
    kw = dict({} if tss is None else {"norm": tss}, **(bins or {}))
    norm = None  # (None: the host front-end as it is)
    if on_device and abundances:  # (a dense table is handed over as the Float64 values the front-end reads; Float32 widens exactly)
        norm = lambda c, t: normalize_abundances(c if (isinstance(c, CSC) or is_device_tensor("normalize_data", c)) else np.asarray(c, dtype=np.float64),
                                                 t, device=device, **kw)
    elif on_device:
        norm = lambda c, t: normalize_counts(c, t, device=device, **kw)
    elif abundances:  # the host front-end with the anchor rule of the Float64 device front-end (preprocess.adaptive_clr)
        norm = lambda c, t: pre.normalize(c, t, prec=prec, tie_anchor=True, **kw)
    elif kw:
        norm = lambda c, t: pre.normalize(c, t, prec=prec, **kw)

    def one(tab, hdr):  # a count table on its own -> (matrix, the kept columns' names, row mask)
        mat, row_mask, col_mask = norm(tab, test_name) if norm else pre.normalize(tab, test_name, prec=prec)
        return mat, [h for h, k in zip(hdr, col_mask) if k], row_mask
    if meta_data is not None:
        r = pre.normalize_with_meta(data, test_name, meta_data, prec=prec, header=header, meta_header=meta_header,
                                    make_onehot=make_onehot, normalizer=norm)
        main = dict(data=r["data"], header=r["header"], meta_mask=np.asarray(r["meta_mask"], dtype=bool), row_mask=r["row_mask"])
    else:
        mat, hdr, row_mask = one(data, header)
        main = dict(data=mat, header=hdr, meta_mask=np.zeros(len(hdr), dtype=bool), row_mask=row_mask)
    if not extra:
        return main, on_device
    tabs, hdrs, masks = zip(*[one(tab, hdr) for tab, hdr in extra])
    mat, hdr, meta_mask, row_mask = pre.combine_data(list(tabs) + [main["data"]], list(hdrs) + [main["header"]],
                                                     [None] * len(extra) + [main["meta_mask"]], list(masks) + [main["row_mask"]])
    return dict(data=mat, header=hdr, meta_mask=meta_mask, row_mask=row_mask), on_device


def _digest_update(h, obj):
    """One argument of learn_network into the hash of the distributed input check: arrays by shape, dtype and bytes, a sparse table by
    its three CSC arrays, containers element by element, anything else by its repr."""
    if _any_sparse(obj):
        colptr, rowval, nzval, shape = _csc_arrays(obj)
        h.update(("csc%r" % (shape,)).encode())
        for a in (colptr, rowval, nzval):
            _digest_update(h, np.asarray(a))
    elif isinstance(obj, np.ndarray):
        h.update(("nd%r%s" % (obj.shape, obj.dtype.str)).encode())
        h.update(repr(obj.tolist()).encode() if obj.dtype.kind == "O" else np.ascontiguousarray(obj).tobytes())
    elif isinstance(obj, (list, tuple)):
        h.update(("seq%d" % len(obj)).encode())
        for v in obj:
            _digest_update(h, v)
    elif hasattr(obj, "__array__") and not isinstance(obj, (str, bytes)):
        _digest_update(h, np.asarray(obj))
    else:
        h.update(("%s:%r" % (type(obj).__name__, obj)).encode())


def _distributed_world():
    """learn_network(distributed=True): the default torch.distributed group must be up -> (torch.distributed, rank, world size)."""
    try:
        import torch.distributed as dist
        up = dist.is_available() and dist.is_initialized()
    except ImportError:
        dist, up = None, False
    if not up:
        raise ValueError("learn_network: distributed=True needs an initialised torch.distributed default group: start the ranks with "
                         "torchrun (or call torch.distributed.init_process_group on every rank) before learn_network; ranks are not "
                         "spawned here")
    return dist, dist.get_rank(), dist.get_world_size()


def _distributed_input_check(dist, rank, world, eng_prec, device, tables, keywords):
    """First step of a sharded learn_network (world > 1), ahead of every other refusal: the one mode without sharded entry points is
    refused, then every rank hashes the arguments that decide the result -- `tables`, the main table first, and the mode `keywords` as
    the caller passed them -- and the ranks compare.  Ranks that disagree on the data would disagree on level 0 and wait for each other
    in a later collective."""
    if eng_prec == 64:
        raise ValueError("learn_network: prec=64 with distributed=True is not supported for the plain fz test: the Float64 mode has no "
                         "sharded entry points (DESIGN.md section 7); run it on one rank or pass prec=32")
    import hashlib
    import torch
    h = hashlib.sha256()
    _digest_update(h, [tables[0] if _any_sparse(tables[0]) else np.asarray(tables[0])] + list(tables[1:]))
    _digest_update(h, sorted(keywords.items()))
    on_gpu = dist.get_backend() == "nccl"  # (a CPU backend compares on the host: no device call before the refusals)
    mine = torch.frombuffer(bytearray(h.digest()), dtype=torch.uint8)
    mine = mine.to(torch.device("cuda", device)) if on_gpu else mine
    everyone = torch.empty(world * mine.numel(), dtype=torch.uint8, device=mine.device)
    dist.all_gather_into_tensor(everyone, mine)
    everyone = everyone.cpu().view(world, -1)
    differ = [r for r in range(world) if not bool((everyone[r] == everyone[0]).all())]
    if differ:
        raise ValueError("learn_network: distributed=True: the ranks were not called with the same arguments -- the digest of the table "
                         "(shape, dtype, bytes) and the mode keywords on rank(s) %s differs from rank 0's (this is rank %d of %d); "
                         "every rank must pass the same data and options, only `device` may differ" % (differ, rank, world))


_Tables = namedtuple("_Tables", "data header meta_data meta_header make_onehot extra mask sparse n_marked")


def _prepare_tables(who, data, header, meta_data, meta_header, make_onehot, extra_data, meta_mask, test_name, prec, device_normalize,
                    normalize, csc_tuple_is_sparse, strict_header, abundances=False):
    """The table stage of both entry points, everything before a front-end or a device sees a table: sparse or dense, the mask vector,
    the sparse refusals, the canonical CSC form, the header, the meta columns split off (normalize=True) or only looked at (a prepared
    matrix keeps them and its mask), the extra tables.  The entry points differ in two rules, which they pass: csc_tuple_is_sparse
    (is an engine.CSC tuple a sparse table?) and strict_header (is a header of another length than the table refused without a mask
    as well?).  abundances (with normalize): a sparse block is made canonical as Float64 instead of as counts, and the value refusals
    come last.  -> _Tables; header is the caller's object when one was given and nothing was split off."""
    dev_csc = is_sparse_csc_tensor(data) and is_device_tensor(who, data)  # a sparse table in GPU memory: canonical as it comes, never touched here
    sparse = (_any_sparse(data) if csc_tuple_is_sparse else is_sparse(data)) or dev_csc
    data = data if (sparse or is_device_tensor(who, data)) else np.asarray(data)  # (a table in GPU memory stays where it is)
    mask = _meta_mask_vector(who, meta_mask, meta_data, data)
    if sparse:
        # a sparse table stays sparse from here to the device (fw_normalize_counts_csc, fw_set_data_csc_*); what would need the dense
        # matrix is refused by name before any device call -- densifying silently would defeat the point
        _sparse_refusals(who, test_name, normalize, prec, device_normalize, meta_data)
    if mask is not None and header is not None and len(header) != _shape(data)[1]:
        raise ValueError("%s: a header of %d names for %d columns%s" % (who, len(header), _shape(data)[1], "" if strict_header else
                         ": with a meta_mask the header names all columns of data, the meta ones included"))
    if mask is None or not normalize:
        data = _canonical_csc(who, data, test_name, normalize, abundances) if (sparse and not dev_csc) else data
        if mask is not None:  # the prepared matrix is taken as it is; its marked columns are only looked at
            _finite_meta(who, pre._csc_take_cols(*data[:3], np.nonzero(mask)[0])[2] if sparse else data[:, mask])
        extra = _extra_tables(who, data, extra_data, test_name, normalize, abundances=abundances)  # (refused by name before any device call)
        if header is None:  # after the extra tables: a call with a bad header AND a bad extra table is told about the table
            header = _default_header(_shape(data)[1])
        elif strict_header and len(header) != _shape(data)[1]:
            raise ValueError("%s: a header of %d names for %d columns" % (who, len(header), _shape(data)[1]))
    else:
        # normalize=True: the meta columns leave the table before anything is checked as a count -- a continuous covariate is no
        # count -- and come back prepared, at its end (preprocessing.jl:425-446,527-558); from here on they are a numeric meta_data
        cols = _shape(data)[1]
        data, header, meta_data, meta_header = _split_meta(who, data, mask, _default_header(cols) if header is None else list(header), test_name,
                                                              abundances)
        make_onehot = False  # (numbers: nothing to encode)
        extra = _extra_tables(who, data, extra_data, test_name, normalize, n_named=cols, abundances=abundances)
    if abundances and normalize:
        _abundance_refusals(who, data, extra)
    return _Tables(data, header, meta_data, meta_header, make_onehot, extra, mask, sparse, 0 if mask is None else int(mask.sum()))


def _resolve_mode(test_name, eng_prec, data, csc_resident, recursive_pcor, dense_cor, who="learn_network", stacklevel=3):
    """The engine options of learn_network against the test kind and the table as the caller gave it: what the CSC-resident layout
    and the Float64 path do not serve is refused, and dense_cor / recursive_pcor become what will run (with the warning, attributed
    to the caller `stacklevel` frames up: that of the entry point `who`).  -> (csc_resident, recursive_pcor, dense_cor)"""
    csc_resident = bool(csc_resident)
    if csc_resident:  # what the CSC-resident layout does not serve is refused by name, never densified
        if test_name != "fz_nz":
            raise ValueError("%s: csc_resident=True is served for sensitive=True, heterogeneous=True (fz_nz) only; the discrete "
                             "kinds are bit-packed already and the plain fz test needs the dense matrix" % who)
        if not (is_sparse(data) or (is_sparse_csc_tensor(data) and is_device_tensor(who, data))):
            raise ValueError("%s: csc_resident=True needs sparse data (a scipy.sparse matrix); a dense table is not "
                             "converted silently" % who)
        if not recursive_pcor:
            raise ValueError("%s: csc_resident=True with recursive_pcor=False is not supported: those conditional tests "
                             "stream whole dense columns" % who)
    if eng_prec == 64 and not (recursive_pcor and dense_cor):
        raise ValueError("%s: prec=64 with %s is not supported: the Float64 path conditions on the resident Float64 "
                         "Pearson matrix (recursive_pcor=True, dense_cor=True)"
                         % (who, "recursive_pcor=False" if not recursive_pcor else "dense_cor=False"))
    if test_name != "fz":
        dense_cor = True  # (learning.jl:42: only the plain fz test ever builds a matrix; the engine takes the flag for fz alone)
    elif not dense_cor and recursive_pcor:
        warnings.warn("%s: dense_cor=False leaves no correlation matrix for recursive partial correlations; "
                      "running with recursive_pcor=False (conditional tests from the data)" % who, stacklevel=stacklevel)
        recursive_pcor = False
    return csc_resident, recursive_pcor, dense_cor


def _matrix(t, test_name, normalize, prec, device_normalize, device, abundances=False):
    """The prepared tables (_Tables) -> (matrix for the engine, header, meta mask as a list or None, normalised on the device?,
    seconds): normalised and combined (normalize=True), prepared tables laid side by side, or the prepared matrix as it is.  The
    seconds are counters["t_normalize_s"]: this step alone."""
    meta_mask = None if t.mask is None else [bool(v) for v in t.mask]  # (normalize=False keeps it; normalize=True returns its own)
    header, on_device, t0 = t.header, False, time.perf_counter()
    if normalize:
        r, on_device = _normalize_tables(t.data, t.header, t.extra, test_name, t.meta_data, t.meta_header, t.make_onehot, prec,
                                         device_normalize, device, abundances)
        mat, header, meta_mask = r["data"], r["header"], [bool(v) for v in r["meta_mask"]]
    elif t.extra:
        # already normalised tables are only laid side by side (learning.jl:537-541): no filter, no alignment, extra tables first
        everyone = np.ones(_shape(t.data)[0], dtype=bool)
        mat, header, combined_mask, _ = pre.combine_data([x for x, _ in t.extra] + [t.data], [h for _, h in t.extra] + [t.header],
                                                         [None] * len(t.extra) + [t.mask], [everyone] * (len(t.extra) + 1))
        meta_mask = None if t.mask is None else [bool(v) for v in combined_mask]
    else:  # the prepared matrix as it is: dense, or Int32 CSC for mi / mi_nz, Float32 CSC for fz_nz
        mat = tuple(t.data[:3]) if (t.sparse and not is_sparse_csc_tensor(t.data)) else t.data
    return mat, header, meta_mask, on_device, time.perf_counter() - t0


def _sharded_lgl(eng, test_name, lgl, dist, rank, world, device):
    """level 0 and lgl of a distributed run on an engine that holds its data: this rank's share, the rounds' neighbour sets exchanged
    in device memory and, with track_rejections, the whole log gathered.  -> (net, what gather_rejections returned or None)"""
    import torch
    from .dist import make_dev_exchange
    xchg = make_dev_exchange(dist, torch.device("cuda", device))
    if test_name in ("mi", "mi_nz"):
        eng.level0_dev(rank, world, xchg)  # this rank's share of the pair tiles
    else:
        eng.level0()  # the Fisher-z kinds stay replicated (include/flashweave_amd.h)
    net = eng.lgl(rank=rank, world_size=world, dev_exchange=xchg, **lgl)
    if not lgl["track_rejections"]:
        return net, None
    gathered = eng.gather_rejections(xchg)  # every rank holds its own targets' records: all of them everywhere
    net["rejections"] = rejections_dict(eng.rejection_records())
    return net, gathered


def _run_engine(mat, n, p, run, dist, rank, world, targets=None):
    """One engine for one run: the matrix goes up, the Pearson matrix is computed where the mode has one, lgl runs single or
    sharded (world > 1) -- or, for learn_neighbors, Engine.neighbors for `targets` (variable ids; one rank) -- the counters are
    read; the engine is closed whatever happens.  run: the entry point's keywords with the resolved values.  -> (net, counters)"""
    test_name = run["test_name"]
    eng = Engine(test_name, n, p, **{k: run[k] for k in _ENGINE_KEYS})
    try:
        # (what the device front-end returned is canonical already: its triple goes up as it is, stored 0.0f of clr_nz included)
        eng.set_data((mat.indptr, mat.indices, mat.data) if is_sparse(mat) else mat, csc_resident=run["csc_resident"])
        if test_name == "fz" and run["dense_cor"]:
            eng.compute_cor()  # (replicated in a distributed run: row-block sharding stays an Engine-level tool, dist.sharded_cor)
        lgl, gathered = {k: run[k] for k in _LGL_KEYS}, None
        if targets is not None:  # (no feed-forward: each neighbourhood on its own; round_size 0 = one batch)
            net = eng.neighbors(targets, edge_dict=True, **{k: run[k] for k in _NEIGHBORS_KEYS})
        elif world > 1:
            net, gathered = _sharded_lgl(eng, test_name, lgl, dist, rank, world, run["device"])
        else:
            net = eng.lgl(**lgl)
        counters = eng.counters()
        counters["world_size"], counters["rank"] = max(world, 1), rank
        for k in ("packed_host", "packed_dev", "received"):  # the log gather of a distributed run (None: there was none)
            counters["rejections_" + k] = None if gathered is None else gathered[k]
        counters["data_resident_bytes"] = eng.data_resident_bytes() if (test_name == "fz_nz" and hasattr(eng.L, "fw_data_resident_bytes")) else None
    finally:
        eng.close()
    return net, counters


def _schedule(round_size, feed_forward, p):
    """parameters["schedule"]: the sentence that says which feed-forward schedule ran."""
    return ("single_il (one target per round: the reference's deterministic schedule)" if round_size == 1
            else "one round (parallel=\"single\": no whitelists)" if (round_size == 0 or not feed_forward or round_size >= p)
            else "rounds of %d targets (whitelists refresh once per round; deviates from single_il)" % round_size)


def _tss_range_refusals(who, norm_mode, data, extra):
    """A TSS norm_mode on tables of real values: every positive value lies in [2^-126, 2^96], so that it does not vanish as a Float32
    and the Float32 sum of a sample (fewer than 2^31 terms) stays finite."""
    for name, tab in [("data", data)] + [("extra_data[%d]" % i, t) for i, (t, _) in enumerate(extra)]:
        defect = tss_range_defect(tab.nzval if isinstance(tab, CSC) else tab.values() if is_sparse_csc_tensor(tab) else tab)
        if defect:
            raise ValueError("%s: norm_mode=%r with abundances=True: %s holds %s" % (who, norm_mode, name, defect))


def normalize_data(data, extra_data=None, test_name=None, header=None, meta_data=None, meta_header=None, make_onehot=True, prec=32,
                   device_normalize=True, device=0, meta_mask=None, abundances=False, norm_mode=None, n_bins=3, rank_method="tied",
                   disc_method="median"):
    """normalize_data (preprocessing.jl:660-701), both forms: what learn_network(normalize=True) does to its tables, as a function of
    its own.  data: samples x OTUs counts (array or scipy.sparse); extra_data: a list of (table, header) pairs, count tables of further
    sequencing experiments on the same samples.  Every table is normalised on its own for `test_name` ("fz" clr_adapt, "fz_nz" clr_nz,
    "mi" presence / absence, "mi_nz" binned_nz_clr) with its own filters; then the samples every table kept are gathered and the
    columns laid out as [last extra, ..., first extra, data (+ meta columns)] (preprocess.combine_data).  All tables take one
    front-end: the device one (integral counts, prec == 32, device_normalize) or, if any table is not integral, the host one.  Sparse
    tables need the device front-end and are refused with what learn_network refuses them with; sparse and dense do not mix.
    meta_mask: one boolean (or 0 / 1) per column of `data`, True marking a meta variable that sits inside the table, dense or sparse
    (see learn_network): the unmarked columns are normalised as the count table, the marked ones prepared like a numeric meta_data
    and appended last; `header` names all columns.
    abundances=True declares the tables real-valued (see learn_network): every table, dense or sparse, takes the Float64 device
    front-end when device_normalize and prec == 32; a NaN, an infinite or a negative value raises ValueError naming abundances and the
    table.
    norm_mode: the reference's other way to choose the transform, by its own names, instead of test_name (giving both raises
    ValueError; giving neither means test_name "fz"): "clr-adapt" = "fz", "clr-nonzero" = "fz_nz", "clr-nonzero-binned" = "mi_nz",
    "pres-abs" = "mi" -- aliases, the same calls and results -- and the two total-sum-scaling modes no test_name selects: "tss"
    (x / the sample's sum over the kept columns, computed in Float{prec} like the reference: Float32 sums in ascending column order;
    dense Float32 or CSC Float32 out, meta variables as for "fz") and "tss-nonzero-binned" (the non-zero TSS values of a column ranked
    into two bins, zeros stay 0: Int32 levels, dense or CSC; meta variables as for "mi_nz").  They take the same front-end choice, host
    and device giving the same bits; with abundances=True a positive value outside [2^-126, 2^96] raises ValueError.  learn_network
    takes such a table with normalize=False.
    n_bins, rank_method, disc_method: the reference's preprocess_kwargs of the two binned modes, test_name "mi_nz" / norm_mode
    "clr-nonzero-binned" and norm_mode "tss-nonzero-binned" (preprocessing.jl:217-291,412-416,492-521).  In every kept column the non-zero
    entries are discretised into n_bins - 1 levels 1 .. n_bins - 1 by their keys (the clr_nz value / the TSS quotient), zeros stay 0:
    disc_method "median" takes the rank r of a key -- rank_method "tied": the average rank, "dense": the distinct keys numbered in
    ascending order -- and level = floor((r / max r) / (1 / (n_bins - 1) + 1e-5)) + 1; disc_method "mean" (n_bins=3 only) gives 1 to
    the keys <= the column's mean and 2 to the others, the mean being preprocess.pairwise_mean of the keys, one number on the host and
    on the device, within rounding of the reference's.  A column is kept iff its non-zero entries show exactly
    n_bins - 1 distinct levels.  Every table of extra_data takes the same options; meta variables go into 2 bins whatever n_bins is.
    Host and device front-end, dense and sparse, counts and abundances give the same levels; learn_network takes the table with
    normalize=False (the discrete engine serves up to 62 levels).  ValueError naming the option, before any device call: n_bins no
    integer in 3 .. 62, an unknown rank_method or disc_method, disc_method="mean" with n_bins > 3, and any of the three away from its
    default with a mode that does not bin.
    data may be a 2-D torch.Tensor in GPU memory (device.type "cuda", on GPU `device`): the device front-end borrows it
    (fw_normalize_counts_dev, with abundances=True fw_normalize_abund_dev) and `data` of the result is a tensor on the same device, an
    (n_out, p_out) view with strides (1, n_out), the bits of the numpy call; header and the two masks come back as always.  Every
    norm_mode and the three binning options are served; meta_data, meta_mask, extra_data, prec=64, device_normalize=False, a
    non-integral tensor without abundances=True, a tensor of another GPU, one that is not 2-D or not numeric and a sparse tensor raise a
    ValueError that names the option and says to pass tensor.cpu() instead (see learn_network).  A sparse CSC tensor in GPU memory
    (layout torch.sparse_csc, canonical: see learn_network) is the sparse table of that path: `data` comes back as a sparse CSC tensor
    on the same device over the front-end's output buffers (a dense tensor for "fz"), the bits of the scipy call.
    -> dict(data, header, meta_mask, row_mask): row_mask over the input samples, data a scipy.sparse.csc_matrix for sparse tables
    (dense for "fz")."""
    who = "normalize_data"
    tss = None
    if norm_mode is not None:
        if test_name is not None:
            raise ValueError("%s: test_name=%r and norm_mode=%r are two ways to choose one transform: give one of them"
                             % (who, test_name, norm_mode))
        if norm_mode not in _NORM_MODES:
            raise ValueError("%s: unsupported norm_mode %r; the modes are %s" % (who, norm_mode, ", ".join(map(repr, _NORM_MODES))))
        test_name = _NORM_MODES[norm_mode]
        if norm_mode in pre.TSS_NORMS:
            tss = norm_mode
    elif test_name is None:
        test_name = "fz"
    if test_name not in _TEST_NAMES:
        raise ValueError("%s: unsupported test_name %r" % (who, test_name))
    if prec not in (32, 64):
        raise ValueError("%s: prec=%r is not supported (32 or 64)" % (who, prec))
    pre.bins_check(who, test_name, n_bins, rank_method, disc_method)
    if is_device_tensor(who, data):  # a table in GPU memory: what would need its bytes on the host is refused by name
        _tensor_refusals(who, data, device, True, bool(abundances), meta_data=meta_data, meta_mask=meta_mask, extra_data=extra_data, prec=prec,
                         device_normalize=device_normalize)
    # this entry point's rules of the table stage: an engine.CSC tuple is a sparse table, and a header always has the table's length
    t = _prepare_tables(who, data, header, meta_data, meta_header, make_onehot, extra_data, meta_mask, test_name, prec, device_normalize,
                        normalize=True, csc_tuple_is_sparse=True, strict_header=True, abundances=bool(abundances))
    if tss is not None and abundances:
        _tss_range_refusals(who, norm_mode, t.data, t.extra)
    return _normalize_tables(t.data, list(t.header), t.extra, test_name, t.meta_data, t.meta_header, t.make_onehot, prec, device_normalize,
                             device, bool(abundances), tss=tss, bins=pre.bins_kw(n_bins, rank_method, disc_method))[0]


def _targets_form(who, targets):
    """learn_neighbors' targets as the caller wrote them: a non-empty list (tuple, 1-D array) that is all names (str) or all integers
    (0-based columns of the main table; booleans are neither) -> "names" or "columns".  Looks at the list alone."""
    if isinstance(targets, (str, bytes)) or not hasattr(targets, "__len__") or getattr(targets, "ndim", 1) != 1:
        raise ValueError("%s: targets must be a list of variable names or of 0-based column indices, got %s" % (who, type(targets).__name__))
    targets = list(targets)
    if not targets:
        raise ValueError("%s: targets is empty: name at least one variable" % who)
    names = [isinstance(v, str) for v in targets]
    columns = [isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in targets]
    if not (all(names) or all(columns)):
        bad = [v for v, a, b in zip(targets, names, columns) if not (a or b)]
        raise ValueError("%s: targets is %s: pass all names (str) or all 0-based column indices (int)"
                         % (who, "a mixed list of names and indices" if not bad else "not a list of names or indices (%r)" % (bad[0],)))
    return "names" if all(names) else "columns"


def _targets_names(who, targets, cols, header):
    """targets -> names: a name stays, a column index of the main table as passed (cols columns) becomes its name under the header in
    effect -- the caller's, or X1 .. -- so that it can be followed through normalisation, which drops and reorders columns."""
    if _targets_form(who, targets) == "names":
        return list(targets)
    header = _default_header(cols) if header is None else [str(h) for h in header]
    bad = [int(v) for v in targets if not 0 <= int(v) < cols]
    if bad:
        raise ValueError("%s: targets holds the column index %d, which is out of range for the %d columns of data (0-based)" % (who, bad[0], cols))
    unnamed = [int(v) for v in targets if int(v) >= len(header)]
    if unnamed:
        raise ValueError("%s: targets holds the column index %d, which the header of %d names does not name" % (who, unnamed[0], len(header)))
    return [header[int(v)] for v in targets]


def resolve_targets(who, names, variable_ids, given=()):
    """learn_neighbors' targets, as names, against the final variable_ids -> their indices there, in the caller's order.  given: the
    names the tables came with (main header, extra headers, meta header): a target among them that variable_ids lacks was dropped by
    normalisation, any other missing one matches nothing.  ValueError naming targets for a name that matches nothing or more than one
    column, two entries that resolve to one variable, and -- all of them listed -- variables normalisation did not keep."""
    where = {}
    for j, h in enumerate(variable_ids):
        where.setdefault(str(h), []).append(j)
    known = set(str(h) for h in given)
    unknown = [v for v in names if v not in where and v not in known]
    if unknown:
        raise ValueError("%s: targets names %r, which matches no variable" % (who, unknown[0]))
    dropped = [v for v in names if v not in where]
    if dropped:
        raise ValueError("%s: targets names %s, which %s not among the variables normalisation kept (a column without enough "
                         "variation is filtered out; normalize_data shows what stays)"
                         % (who, ", ".join(repr(v) for v in dict.fromkeys(dropped)), "is" if len(set(dropped)) == 1 else "are"))
    twice = [v for v in names if len(where[v]) > 1]
    if twice:
        raise ValueError("%s: targets names %r, which matches %d columns (%s): variable names must be unique to be targets"
                         % (who, twice[0], len(where[twice[0]]), ", ".join(map(str, where[twice[0]]))))
    ids = [where[v][0] for v in names]
    if len(set(ids)) != len(ids):
        again = next(v for i, v in enumerate(names) if v in names[:i])
        raise ValueError("%s: targets lists the variable %r twice: every target once" % (who, again))
    return ids


def learn_neighbors(data, targets, meta_data_path=None, *, sensitive=True, heterogeneous=False, max_k=3, alpha=0.01, normalize=True,
                    header=None, hps=5, FDR=True, n_obs_min=-1, max_tests=10_000_000, prec=32, device=0, meta_data=None, meta_header=None,
                    make_onehot=True, recursive_pcor=True, dense_cor=True, device_normalize=True, fast_elim=True, no_red_tests=True,
                    track_rejections=False, csc_resident=False, extra_data=None, transposed=False, meta_mask=None, abundances=False,
                    **unsupported):
    """si_HITON_PC(T, data; test_name, ...) (src/hiton.jl:402-409) for a list of targets: the direct neighbourhoods of chosen
    variables without learning the whole network.  Level 0 runs over all pairs with Benjamini-Hochberg as in learn_network; HITON-PC
    then runs for the listed targets only, each on its own (no feed-forward: the reference passes an empty whitelist).
    data, meta_data_path and every keyword mean what they mean for learn_network, with the same table forms (numpy, scipy.sparse,
    dense and sparse CSC tensors in GPU memory, extra_data, meta_data / meta_mask, the path form, abundances, csc_resident, prec=64)
    and the same refusals, under this function's name.  feed_forward, round_size and distributed are not taken: there is no schedule
    to choose and no sharded form; they raise TypeError like any unknown keyword.
    targets: a non-empty list, all names or all integers.  Names (str) are looked up in the final variable_ids.  Integers are 0-based
    columns of the main `data` as passed; they are translated through the header in effect (the caller's, or X1 ..) and then looked
    up the same way, so that a column normalisation dropped in front of a target does not shift it.  ValueError naming targets,
    before any engine is created: an empty or a mixed list, a name that matches nothing or more than one column, an index out of
    range, two entries that resolve to one variable, and variables normalisation did not keep (all of them are listed).
    -> FWResult with learn_network's keys and
        targets      the resolved indices into variable_ids, in the caller's order
        neighbors    {target index: {neighbour index: (weight, pval)}}: HITON-PC's result for the target, in PC order
    A target's neighbours are those of its row in learn_network(..., feed_forward=False), weight and p to the bit.  edges is
    make_symmetric_graph of the targets' rows alone: an edge between two targets is merged as always, an edge to another variable
    has the target's direction only.  rejections (track_rejections=True) holds the targets' records.  parameters["targets"] is their
    number and parameters["schedule"] says that every neighbourhood ran on its own.  save and save_rejections work unchanged."""
    if unsupported:
        raise TypeError("learn_neighbors: unsupported options %s (see DESIGN.md section 7)" % sorted(unsupported))
    _targets_form("learn_neighbors", targets)
    return _learn("learn_neighbors", list(targets), data, meta_data_path, transposed, False, dict(
        sensitive=sensitive, heterogeneous=heterogeneous, max_k=max_k, alpha=alpha, feed_forward=False, normalize=normalize,
        hps=hps, FDR=FDR, n_obs_min=n_obs_min, max_tests=max_tests, prec=prec, round_size=0, make_onehot=make_onehot,
        recursive_pcor=recursive_pcor, dense_cor=dense_cor, device_normalize=device_normalize, fast_elim=fast_elim,
        no_red_tests=no_red_tests, track_rejections=track_rejections, csc_resident=csc_resident, abundances=abundances),
        dict(header=header, meta_data=meta_data, meta_header=meta_header, extra_data=extra_data, meta_mask=meta_mask), device)


def learn_network(data, meta_data_path=None, *, sensitive=True, heterogeneous=False, max_k=3, alpha=0.01, feed_forward=True, normalize=True,
                  header=None, hps=5, FDR=True, n_obs_min=-1, max_tests=10_000_000, prec=32, round_size=None, device=0,
                  meta_data=None, meta_header=None, make_onehot=True, recursive_pcor=True, dense_cor=True, device_normalize=True, fast_elim=True,
                  no_red_tests=True, track_rejections=False, csc_resident=False, extra_data=None, transposed=False, meta_mask=None, distributed=False,
                  abundances=False, **unsupported):
    """data: samples x OTUs count matrix (or an already normalised matrix with normalize=False); a numpy array or a scipy.sparse
    matrix.  A sparse table stays sparse end to end (what the reference does with make_sparse, learning.jl:470): normalize=True runs
    the device CSC front-end (integer counts only) and the sparse upload, normalize=False uploads the matrix as it is (Int32 levels
    for mi / mi_nz, Float32 clr_nz values for fz_nz); counters["sparse_input"] records it.  Sparse data is refused (ValueError) with
    device_normalize=False, prec=64, meta_data, and for the plain fz test with normalize=False: each of those needs the dense matrix.
    meta_data: optional samples x meta-variables table (numbers and / or string factors), handled like the reference's
    meta_data_path input: one-hot encoding, discretisation for the discrete tests, +1 shift for fz_nz (preprocess.py).
    round_size: targets per feed-forward round.  None (default) = default_round_size(p): the reference's `single_il` schedule
    (1) up to 512 variables, eight to ten device rounds per pass beyond (the benchmarked configuration; the whitelists refresh
    once per round).  1 = `single_il` at any size (what the golden networks were generated with): every round is one target
    and runs through the host job pool -- exact reproduction of the reference's edge lists, and far slower on large tables.
    0 = one round (parallel="single").
    recursive_pcor / dense_cor (sensitive mode, learning.jl:42,127): recursive_pcor=False takes the conditional tests from the data
    instead of the Pearson matrix; dense_cor=False never builds the p x p matrix at all -- level 0 multiplies and screens the
    centred columns tile by tile (same network as dense_cor=True, memory bounded by the data).  As in the reference, dense_cor
    only matters for the plain "fz" test (the other tests never build a matrix: the flag is ignored there); without a matrix the
    conditional tests can only come from the data, so dense_cor=False implies recursive_pcor=False (a warning says so when the
    caller left recursive_pcor at its default).
    device_normalize: normalise integer count tables on the device (fw_normalize_counts; all four modes); False, or a table of
    non-integral abundances, takes the host front-end (preprocess.py).
    fast_elim (learning.jl:430,469): False runs HITON-PC's exact elimination phase -- a member that fails its test stays in the
    conditioning pool of the later members (hiton.jl:67-70).  no_red_tests (an LGL keyword, learning.jl:207): with fast_elim=False,
    no_red_tests=False keeps the elimination-phase statistics in PC (hiton.jl:388-390); with fast_elim=True it has no effect.
    track_rejections (learning.jl:446,469): True also returns, for every candidate a conditional test removed from a target's
    neighbourhood, the conditioning set that did it: result["rejections"] = {target: {candidate: (Zs, (stat, pval, df, suff_power),
    (num_tests, frac))}} with 0-based variable ids (the reference's rejections(net_result)); {} when off.  io.save_rejections writes
    them in the reference's file format.
    prec (learning.jl:42-45, cont_type): 32 or 64 (16 and 128 are not served).  With the plain "fz" test, prec=64 runs the whole
    continuous pipeline in Float64 on the device: the Pearson matrix, level 0 and pcor_rec with its five-digit rounding (what the
    reference's golden networks were generated with); it needs recursive_pcor=True and dense_cor=True.  "fz_nz" keeps Float32 values
    with Float64 arithmetic whatever prec says, and the discrete tests have no element type: parameters["prec"] records what ran.
    csc_resident (default False): True keeps a sparse fz_nz table sparse on the device as well -- the bit plane, one 32-bit position
    per plane word and the values != 0 (12 p ceil(n / 64) + 4 nnz bytes) instead of the n x p Float32 matrix -- for tables whose dense
    form does not fit; the network is the same to the bit, the tests read each value through two more loads.  It needs sparse data,
    sensitive=True, heterogeneous=True and recursive_pcor=True; anything else is refused (ValueError) before any device call.
    counters["csc_resident"] and counters["data_resident_bytes"] (fz_nz only, else None) record what ran.
    extra_data (learning.jl:460,497-541): a list of (table, header) pairs -- count tables of further sequencing experiments (16S + ITS)
    on the same samples, same rows in the same order; header None numbers the columns on from the main table's.  normalize=True
    normalises every table on its own (normalize_data: its own row sums, geometric means, pseudo-counts and filters -- what stacking
    the tables first would not do), keeps the samples every table kept (a warning says how many were dropped) and lays the columns out
    as [last extra, ..., first extra, data, meta columns]: that order numbers the variables.  normalize=False only lays the prepared
    tables side by side in that order.  meta_data belongs to the main table.  All tables are dense or all sparse, and all take one
    front-end (if any table is not integral, all take the host one).  A table with another number of rows, a header of another length,
    a sparse / dense mix and an entry that is no pair raise ValueError naming extra_data before any device call.
    counters["n_tables"] and parameters["extra_data"] record the count; t_normalize_s covers all tables.
    meta_mask (learning.jl:468,502-504, preprocessing.jl:425-446,527-558): meta variables inside `data` -- one boolean (or 0 / 1) per
    column, True marking a meta variable, anywhere in the table; `header`, when given, names all columns.  This is the form a sparse
    table carries its meta variables in, and the form a prepared matrix carries its mask in.  normalize=True: the unmarked columns
    are the count table, normalised exactly as without a mask (one front-end per run, chosen by the OTU block alone); the marked
    columns get what a numeric meta_data gets (they follow the row mask, continuous ones are discretised into 2 bins for mi / mi_nz,
    columns holding a zero are shifted by +1 for fz_nz, zero-variance ones are dropped) and come LAST: [kept OTU columns, kept meta
    columns], variable_ids and meta_variable_mask to match.  A sparse table is split on its CSC arrays before the count check (a
    continuous covariate is no count), the few meta columns alone are densified on the host, and the result stays CSC (Int32 levels,
    a zero level absent; Float32 for fz_nz); csc_resident=True works on it as on any sparse table.  normalize=False: the matrix is
    taken as it is, dense or sparse, columns neither reordered nor filtered, and the mask goes into meta_variable_mask.  With
    extra_data the mask belongs to the main table.  The marked columns are numbers, so make_onehot has nothing to encode: string
    factors keep going through meta_data (dense tables only).  meta_mask with meta_data, with the path form (files bring
    meta_data_path), of another length than the table has columns, with entries other than booleans or 0 / 1, marking every column,
    or marking a column with a non-finite value raises ValueError naming meta_mask before any device call; an all-False mask is no
    mask.  parameters["meta_mask"] records the number of marked columns.
    distributed (default False): True runs the call SPMD over the ranks of an already initialised torch.distributed default group
    (the reference's workers, learning.jl:130-199, as one process per GPU): every rank calls learn_network with the same arguments, each
    with its own `device`, and every rank gets the same FWResult.  Results do not depend on the number of ranks.  First the ranks
    compare a digest of the table (shape, dtype, bytes; a sparse table's three CSC arrays) and of the mode keywords: a mismatch
    raises ValueError naming distributed on every rank instead of a deadlock later.  Then every rank normalises for itself (the
    front-ends are deterministic: all four modes, sparse tables, extra_data, meta_mask, the path form and csc_resident stay available),
    level 0 of the discrete kinds screens this rank's share of the pair tiles (the Fisher-z kinds stay replicated, as does the Pearson
    matrix), the targets of every feed-forward round are dealt to the ranks, the round's neighbour sets are exchanged in device
    memory (dist.make_dev_exchange) and, with track_rejections, the rejection log is gathered the same way
    (Engine.gather_rejections), so that result["rejections"] is the whole log everywhere.  Ranks are not spawned here:
        torchrun --nproc-per-node 8 run.py          # run.py:
        torch.distributed.init_process_group("nccl")
        net = learn_network(counts, distributed=True, device=int(os.environ["LOCAL_RANK"]))
    Without an initialised group: ValueError naming distributed, before any device call; a world of one rank takes the ordinary path.
    prec=64 with the plain fz test is refused (ValueError naming prec=64 and distributed): the Float64 mode has no sharded entry points.
    parameters["distributed"] records the world size (0 when off), counters["world_size"] and counters["rank"] the rank's place; the
    other counters are the rank's own.
    abundances (default False): True declares the tables real-valued -- relative abundances, percentages, coverage-normalised counts,
    counts beyond 2^31 - 1 -- as the reference normalises any Real matrix (adaptive_pseudocount!: a smallest abundance below 1 sets the
    floor at a tenth of it).  Every table -- the main one, each of extra_data, the OTU block under a meta_mask -- then takes the Float64
    device front-end (engine.normalize_abundances) when device_normalize and prec == 32, dense or sparse; whether a table is integral
    is not asked, and a sparse block is made canonical as Float64.  A dense table with device_normalize=False or prec=64 goes to the
    host front-end, a sparse one keeps its refusals.  abundances=True with normalize=False (nothing to normalise) and a NaN, an
    infinite or a negative value in a table (named: data or extra_data[i]) raise ValueError naming abundances before any device call.
    Without the option a real-valued dense table goes to the host front-end and a sparse one is refused, as before.
    parameters["abundances"] is there (True) only when the option is on.
    A table in GPU memory: data may be a 2-D torch.Tensor with device.type "cuda" on GPU `device`.  It never crosses to the host: the
    front-end borrows it and writes into a device buffer (engine.normalize_counts / normalize_abundances: fw_normalize_*_dev), and the
    engine builds its resident layout from that buffer on the device (Engine.set_data: fw_set_data_dense_*_dev); normalize=False hands
    the tensor straight to the engine.  The result is the FWResult of tensor.cpu().numpy(), to the bit; counters["table_on_device"] and
    parameters["table_on_device"] are there (True) only for such a call.  All four tests, abundances=True, header and every engine
    option are served.  Refused with a ValueError that names the option and says to pass tensor.cpu() instead, before any library
    call: meta_data, meta_mask, extra_data, prec=64, device_normalize=False, distributed=True, csc_resident=True, a non-integral tensor
    without abundances=True, a tensor of another GPU than `device`, one that is not 2-D or not numeric, a sparse tensor.  A CPU tensor
    is an array (np.asarray); any other device type raises ValueError.
    A sparse table in GPU memory: a 2-D tensor with layout torch.sparse_csc (what torch.sparse_csc_tensor builds over a canonical
    scipy triple moved to the GPU) is the sparse form of that path, for every test, abundances=True included.  Its three arrays are
    borrowed where they lie (fw_normalize_counts_csc_dev / fw_normalize_abund_csc_dev write the output triple into device buffers,
    fw_set_data_csc_i32_dev / fw_set_data_csc_f32_dev / fw_set_data_csc_f32_resident_dev build the resident layout from them); of the
    table only the p + 1 column pointers and the front-end's small per-column and per-row records reach the host.  The result is the
    FWResult of the same table as a scipy.sparse.csc_matrix, to the bit, with counters["sparse_input"], counters["table_on_device"]
    and parameters["table_on_device"] all True.  It gets the refusals of a dense device tensor -- the same option names, the same way
    out -- except csc_resident=True, which is served for fz_nz as for scipy, and the sparse refusal of sensitive=True,
    heterogeneous=False, normalize=False.  Unlike a scipy matrix it is not made canonical (no duplicates summed, stored zeros
    dropped or rows sorted on the device): it must be canonical already, and one that is not raises FlashWeaveError naming the column
    (ValueError when the column pointers themselves do not run from 0 to the number of entries); for fz_nz with normalize=False a
    stored 0.0 is an absence.  Every other sparse layout (COO, CSR, BSR, BSC) stays refused: tensor.to_sparse_csc() converts.
    Path form (learning.jl:354-401): data may be a path (str / os.PathLike) or a list of paths, read with io.load_data (.tsv, .csv,
    BIOM 1.0 JSON; anything else raises what load_data raises): the first is the main table, the others become extra_data under their
    file headers; meta_data_path (second positional argument, as in the reference) is the main table's meta data file;
    transposed=True reads every file as variables x samples.  Every other option is a keyword.  meta_data_path or transposed with an
    array raise ValueError."""
    if unsupported:
        raise TypeError("learn_network: unsupported options %s (see DESIGN.md section 7)" % sorted(unsupported))
    return _learn("learn_network", None, data, meta_data_path, transposed, distributed, dict(
        sensitive=sensitive, heterogeneous=heterogeneous, max_k=max_k, alpha=alpha, feed_forward=feed_forward, normalize=normalize,
        hps=hps, FDR=FDR, n_obs_min=n_obs_min, max_tests=max_tests, prec=prec, round_size=round_size, make_onehot=make_onehot,
        recursive_pcor=recursive_pcor, dense_cor=dense_cor, device_normalize=device_normalize, fast_elim=fast_elim,
        no_red_tests=no_red_tests, track_rejections=track_rejections, csc_resident=csc_resident, abundances=abundances),
        dict(header=header, meta_data=meta_data, meta_header=meta_header, extra_data=extra_data, meta_mask=meta_mask), device)


def _learn(who, targets, data, meta_data_path, transposed, distributed, mode, tables, device):
    """The body learn_network and learn_neighbors share, one frame below either: mode holds the mode keywords as the caller passed
    them (what the ranks of a distributed run compare), tables the arguments that describe the tables (header, meta_data, meta_header,
    extra_data, meta_mask).  targets is None for learn_network; for learn_neighbors it is the caller's list, already checked for its
    form (_targets_form), and is resolved against the final variable_ids before an engine exists (resolve_targets)."""
    header, meta_data, meta_header, extra_data, meta_mask = (tables[k] for k in ("header", "meta_data", "meta_header", "extra_data", "meta_mask"))
    normalize, prec, device_normalize, csc_resident = mode["normalize"], mode["prec"], mode["device_normalize"], mode["csc_resident"]
    if prec not in (32, 64):
        raise ValueError("%s: prec=%r is not supported (32 or 64; the reference's 16 and 128 are not served)" % (who, prec))
    abundances = mode["abundances"] = bool(mode["abundances"])  # (before the digest: ranks passing 1 and True make the same run)
    on_gpu = is_device_tensor(who, data)
    if on_gpu:  # a table in GPU memory: what would need its bytes on the host is refused by name, before any library call
        if abundances and not normalize:
            raise ValueError("%s: abundances=True with normalize=False is not supported: the option chooses the front-end of a "
                             "table that is normalised here, and a prepared matrix has nothing left to normalise" % who)
        _tensor_refusals(who, data, device, normalize, abundances, meta_data=meta_data, meta_mask=meta_mask, extra_data=extra_data,
                         prec=prec, device_normalize=device_normalize, distributed=distributed, csc_resident=csc_resident)
    caller = mode  # the mode keywords as the caller passed them, before any is resolved
    data, header, meta_data, meta_header, extra_data = _path_form(data, meta_data_path, transposed, header, meta_data, meta_header, meta_mask,
                                                                  extra_data, who=who)
    test_name = ("fz" if mode["sensitive"] else "mi") + ("_nz" if mode["heterogeneous"] else "")  # src/learning.jl:480-483
    eng_prec = 64 if (prec == 64 and test_name == "fz") else 32  # the element type of the device pipeline
    dist, rank, world = _distributed_world() if distributed else (None, 0, 0)
    if world > 1:  # a sharded run (a world of one rank takes the ordinary path): its refusals first, the same on every rank
        _distributed_input_check(dist, rank, world, eng_prec, device, (data, meta_data, meta_header, header, meta_mask, extra_data), caller)
    # (the warning of _resolve_mode goes to the caller of the entry point: this frame, the entry point's, then theirs)
    csc_resident, recursive_pcor, dense_cor = _resolve_mode(test_name, eng_prec, data, csc_resident, mode["recursive_pcor"], mode["dense_cor"],
                                                            who=who, stacklevel=4)
    # the entry points' rules of the table stage: an engine.CSC tuple is no sparse table here, and without a mask a header of
    # another length than the table passes (zip truncates)
    if abundances and not normalize:
        raise ValueError("%s: abundances=True with normalize=False is not supported: the option chooses the front-end of a "
                         "table that is normalised here, and a prepared matrix has nothing left to normalise" % who)
    if targets is not None:  # the names of the main table's columns as passed: what an integer target is translated through
        cols = _shape(data if (_any_sparse(data) or is_device_tensor(who, data)) else np.asarray(data))
        named = _targets_names(who, targets, cols[1] if len(cols) == 2 else 0, header)
    t = _prepare_tables(who, data, header, meta_data, meta_header, mode["make_onehot"], extra_data, meta_mask, test_name, prec,
                        device_normalize, normalize=normalize, csc_tuple_is_sparse=False, strict_header=False, abundances=abundances)
    if meta_data is not None and not normalize:
        # the reference appends the meta columns as they are and keeps their mask (learning.jl:500-520); here an already
        # normalised matrix must already hold them -- silently dropping the argument would lose the mask
        raise ValueError("%s: meta_data with normalize=False is not supported: append the prepared meta columns to "
                         "`data` yourself (preprocess.normalize_with_meta) and mark them with meta_mask, or pass normalize=True" % who)
    mat, header, meta_mask, on_device, t_norm = _matrix(t, test_name, normalize, prec, device_normalize, device, abundances)
    n, p = t.data[3] if isinstance(mat, tuple) else mat.shape
    ids = None
    if targets is not None:  # before an engine exists: a bad list costs no device call beyond the front-end's
        given = list(t.header) + [h for _, hdr in t.extra for h in hdr] + [str(h) for h in (t.meta_header if t.meta_header is not None else [])]
        ids = resolve_targets(who, named, header, given)
    run = dict(caller, device=device, test_name=test_name, prec=eng_prec, csc_resident=csc_resident, recursive_pcor=recursive_pcor,
               dense_cor=dense_cor, round_size=default_round_size(p) if mode["round_size"] is None else mode["round_size"])
    net, counters = _run_engine(mat, n, p, run, dist, rank, world, targets=ids)
    counters.update(t_normalize_s=t_norm, normalized_on_device=on_device, sparse_input=t.sparse, n_tables=1 + len(t.extra),
                    csc_resident=csc_resident)
    parameters = {k: bool(run[k]) if k in ("fast_elim", "no_red_tests", "track_rejections") else run[k] for k in _REPORTED}
    parameters.update(extra_data=len(t.extra), meta_mask=t.n_marked, distributed=world, schedule=_schedule(run["round_size"], mode["feed_forward"], p))
    if abundances:
        parameters["abundances"] = True
    if on_gpu:  # (the table never left the device: front-end and upload borrowed it there)
        counters["table_on_device"] = parameters["table_on_device"] = True
    res = FWResult(edges=net["edges"], variable_ids=header, meta_variable_mask=meta_mask or [False] * len(header), parameters=parameters,
                   counters=counters, rejections=net["rejections"])
    if targets is not None:
        off, idx, w, pv = net["pc_off"], net["pc_idx"].tolist(), net["pc_weight"].tolist(), net["pc_pval"].tolist()
        parameters.update(targets=len(ids), schedule="targets (no feed-forward: each neighbourhood on its own)")
        res["targets"] = list(ids)
        res["neighbors"] = {v: {idx[q]: (w[q], pv[q]) for q in range(int(off[v]), int(off[v + 1]))} for v in ids}
    return res
