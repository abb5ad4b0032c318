"""Host-side normalisation front-end: the three modes the BASELINE configs use.

Mirrors preprocess_data (reference src/preprocessing.jl:412-563) for a plain count matrix without meta
variables: variance / zero-read filters (:367-409), then
  "fz"    -> clr_adapt      adaptive pseudo-counts + centred log-ratio (:133-214)      -> Float32 dense
  "mi"    -> binary         presence/absence, columns with exactly 2 levels (:475-490) -> int {0,1}
  "mi_nz" -> binned_nz_clr  non-zero CLR, 2-bin median discretisation of the non-zeros (:492-521) -> int {0,1,2}
                            (n_bins, rank_method, disc_method: other numbers of bins, dense ranks, the "mean" rule; discretize_nz)
Computation is in Float64 like the reference (clrnorm converts to Matrix{Float64}, :330-341); `prec` only
selects the output type of the continuous mode (convert_to_target_prec, misc.jl:54-62).
The two total-sum-scaling modes (normalize(norm=...), TSS_NORMS) are the exception: like the reference they compute in
Float{prec} (tss()).
"""
import numpy as np


def filter_by_variance(data):
    """preprocessing.jl:367-409: drop zero-variance columns, then all-zero rows."""
    col_mask = np.var(data, axis=0) > 0.0
    data = data[:, col_mask]
    row_mask = data.sum(axis=1) > 0
    return data[row_mask, :], row_mask, col_mask


def adaptive_clr(counts, tie_anchor=False):
    """clr_adapt for a dense count matrix (what preprocessing.jl:157-214 computes): every sample's zeros are replaced by ONE fill value
    chosen so that the filled sample is as far from its own geometric mean as the deepest sample is when ITS zeros hold the floor
    value -- in logs,  fill_i = exp( [ (z* - w) log(floor) + L* - L_i ] / (z_i - w) )  with z = zeros of the sample, L = sum of the logs
    of its non-zero counts, w = the table's width, * = the sample with the largest total -- followed by the centred log-ratio.
    The sample with the largest total is the first of maximal Float64 sum, as in the reference (findmax, preprocessing.jl:158).
    tie_anchor=True (what abundances=True asks for, and what the device front-end does for real values): sums within width * 2^-52 of
    the largest take part as well, and the first of those samples is the anchor.  In a table of relative abundances every sample
    sums to 1 up to rounding and the plain rule is decided by the order of the additions; the window is the rounding bound
    (width - 1) * 2^-53 of a sum of `width` non-negative terms in any order, taken on either side.  It makes the choice independent of
    the order unless a sample's true depth lies about one bound below the maximum, where it can still go either way.
    Returns (matrix, kept-samples mask); a sample whose fill value underflows to zero is dropped."""
    M = np.array(counts, dtype=np.float64)
    n_samples, width = M.shape
    present = M != 0
    zeros = width - present.sum(axis=1)
    if (zeros >= width).any():
        raise ValueError("samples with all zero abundances are not allowed")
    log_mass = np.array([np.log(M[i, present[i]]).sum() for i in range(n_samples)])
    depth = M.sum(axis=1)
    deepest = int(np.argmax(depth >= depth.max() * (1.0 - width * 2.0 ** -52))) if tie_anchor else int(np.argmax(depth))
    smallest = M[present].min()
    floor = 1.0 if smallest >= 1 else smallest / 10
    anchor = (zeros[deepest] - width) * np.log(floor) + log_mass[deepest]
    fill = np.exp((1.0 / (zeros - width)) * (anchor - log_mass))
    kept = fill != 0
    M, present, fill = M[kept], present[kept], fill[kept]
    M = np.where(present, M, fill[:, None])
    centre = np.exp(np.log(M).mean(axis=1, keepdims=True))  # geometric mean of the filled sample
    return np.log(M / centre), kept


def clr_nz(X):
    """clr!(ignore_zeros=true) (preprocessing.jl:192-207): log(x / geomean of the row's non-zeros), zeros stay 0."""
    X = np.array(X, dtype=np.float64)
    out = np.zeros_like(X)
    for i in range(X.shape[0]):
        m = X[i] != 0
        if m.any():
            g = np.exp(np.log(X[i, m]).mean())
            out[i, m] = np.log(X[i, m] / g)
    return out


def _tiedrank(x):
    from scipy.stats import rankdata
    return rankdata(x, method="average")


def _denserank(x):
    from scipy.stats import rankdata
    return rankdata(x, method="dense").astype(np.float64)


def pairwise_mean(keys):
    """The threshold of disc_method "mean", the one number the host and both device forms compute: the keys sorted ascending, padded
    with +0.0 to the next power of two, added level by level (a[2i] + a[2i+1]), divided by their number.  Within rounding of the
    reference's mean(x_vec) (preprocessing.jl:263), which leaves the order of its additions to Base."""
    a = np.sort(np.asarray(keys, dtype=np.float64))
    m, size = a.size, 1
    while size < m:
        size *= 2
    a = np.concatenate([a, np.zeros(size - m)])
    while a.size > 1:
        a = a[0::2] + a[1::2]
    return a[0] / m


RANK_METHODS, DISC_METHODS = ("tied", "dense"), ("median", "mean")
N_BINS_MAX = 62  # the engine takes variables of at most 62 levels (0 .. 61)


def bins_check(who, test_name, n_bins=3, rank_method="tied", disc_method="median"):
    """The three options of the binned modes (preprocessing.jl:217-291,412-416) against each other and against the test_name the
    transform goes with ("mi_nz": binned_nz_clr and, with norm "tss-nonzero-binned", binned_nz_rows); anything else raises ValueError
    naming the option.  -> True when all three are at their defaults."""
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or not 3 <= n_bins <= N_BINS_MAX:
        raise ValueError("%s: n_bins=%r is not supported: an integer in 3 .. %d (two levels are \"mi\" / \"pres-abs\"; the engine takes "
                         "variables of at most %d levels)" % (who, n_bins, N_BINS_MAX, N_BINS_MAX))
    if rank_method not in RANK_METHODS:
        raise ValueError("%s: rank_method=%r is not a valid ranking method (%s)" % (who, rank_method, ", ".join(map(repr, RANK_METHODS))))
    if disc_method not in DISC_METHODS:
        raise ValueError("%s: disc_method=%r is not a valid discretization method (%s)" % (who, disc_method, ", ".join(map(repr, DISC_METHODS))))
    if disc_method == "mean" and n_bins > 3:
        raise ValueError("%s: disc_method='mean' only works with 2 non-zero bins (n_bins=3), got n_bins=%d" % (who, n_bins))
    default = n_bins == 3 and rank_method == "tied" and disc_method == "median"
    if not default and test_name != "mi_nz":
        given = "n_bins=%r" % (n_bins,) if n_bins != 3 else "rank_method=%r" % (rank_method,) if rank_method != "tied" else "disc_method=%r" % (disc_method,)
        raise ValueError("%s: %s applies to the binned modes only (test_name \"mi_nz\" / norm_mode \"clr-nonzero-binned\", "
                         "\"tss-nonzero-binned\"), not to %r" % (who, given, test_name))
    return default


def bins_kw(n_bins=3, rank_method="tied", disc_method="median"):
    """The three options as keywords for the next layer, only those away from their defaults: a call at the defaults is handed on as it
    always was."""
    given = dict(n_bins=n_bins, rank_method=rank_method, disc_method=disc_method)
    return {k: v for k, v in given.items() if v != dict(n_bins=3, rank_method="tied", disc_method="median")[k]}


def discretize_nz(col, nz_mask, n_bins=3, rank_method="tied", disc_method="median"):
    """discretize_nz + discretize (preprocessing.jl:238-291) of the column's non-zero entries into n_bins - 1 levels 1 .. n_bins - 1,
    zeros stay 0.  "median": the tied (average) or the dense rank r, level = floor((r / max r) / (1 / (n_bins - 1) + 1e-5)) + 1;
    "mean" (n_bins = 3): level = 1 where the value is <= pairwise_mean of the non-zero entries, 2 above it."""
    bins_check("discretize_nz", "mi_nz", n_bins, rank_method, disc_method)
    out = np.zeros(col.shape[0], dtype=np.int64)
    if nz_mask.any() and disc_method == "mean":
        out[nz_mask] = np.where(col[nz_mask] <= pairwise_mean(col[nz_mask]), 1, 2)
    elif nz_mask.any():
        r = _tiedrank(col[nz_mask]) if rank_method == "tied" else _denserank(col[nz_mask])
        r = r / r.max()
        step = (1.0 / (n_bins - 1)) + 1e-5
        out[nz_mask] = np.floor(r / step).astype(np.int64) + 1
    return out


# ---- meta variables (preprocessing.jl:42-117 one-hot, :293-316 discretize_meta!, :527-555) ---------------------------------
def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def onehot(meta, header=None):
    """onehot(X, vnames) (preprocessing.jl:42-117): a string factor with more than two categories becomes one 0/1 dummy
    column per category (sorted, named <var>_<category>); a string factor with one or two categories becomes the integers
    1, 2 (factors_to_ints); numeric columns pass through.  -> (Float64 matrix, header)"""
    meta = np.asarray(meta, dtype=object)
    cols, names = [], []
    for j in range(meta.shape[1]):
        x = meta[:, j]
        name = header[j] if header is not None else ""
        if _is_number(x[0]):
            cols.append(np.array([float(v) for v in x]))
            names.append(name)
            continue
        cats = sorted(set(x))
        if len(cats) > 2:
            for cat in cats:
                cols.append(np.array([1.0 if v == cat else 0.0 for v in x]))
                names.append("%s_%s" % (name, cat) if name else "")
        else:
            fmap = {c: float(i + 1) for i, c in enumerate(cats)}
            cols.append(np.array([fmap[v] for v in x]))
            names.append(name)
    return np.stack(cols, axis=1), names


def is_continuous_vec(x):
    """iscontinuous(x_vec) (preprocessing.jl:295-302)."""
    if np.allclose(np.round(x), x):
        return bool(x.max() > 1 or len(np.unique(x)) > 2)
    return True


def discretize(x, n_bins):
    """discretize(x_vec, n_bins), disc_method = "median", rank_method = "tied" (preprocessing.jl:238-265)."""
    if len(x) == 0:
        return x
    r = _tiedrank(x)
    r = r / r.max()
    step = (1.0 / n_bins) + 1e-5
    return np.floor(r / step)


def prepare_meta_block(md, mh, test_name, row_mask):
    """What preprocess_data does to the meta block (preprocessing.jl:527-558), for both ways the block arrives (a meta_data table,
    or the columns a meta_mask marks in `data`): md, a samples x meta-variables Float64 matrix, follows the row mask of the OTU
    normalisation; columns that look continuous are discretised into 2 bins for the discrete tests; columns holding a zero are shifted
    by +1 for "fz_nz" (zeros mean "absent" there); zero-variance columns are dropped.  The caller's matrix is left alone.
    A TSS norm comes with the test_name it goes with (TSS_NORMS): "tss" with "fz" -- a continuous norm, nothing is discretised or
    shifted -- and "tss-nonzero-binned" with "mi_nz" -- discretised, not shifted.
    -> (Float64 matrix, names)"""
    md = md[row_mask]
    if test_name in ("mi", "mi_nz"):
        for j in range(md.shape[1]):
            if is_continuous_vec(md[:, j]):
                md[:, j] = discretize(md[:, j], 2)
    if test_name == "fz_nz":
        for j in range(md.shape[1]):
            if (md[:, j] == 0).any():
                md[:, j] += 1
    keep = np.var(md, axis=0) > 0.0
    return md[:, keep], [h for h, k in zip(mh, keep) if k]


def normalize_with_meta(counts, test_name, meta, prec=32, header=None, meta_header=None, make_onehot=True, normalizer=None, norm=None,
                        n_bins=3, rank_method="tied", disc_method="median"):
    """preprocess_data with a meta_mask (preprocessing.jl:412-563): OTU columns are normalised as in normalize(); meta
    variables are one-hot encoded, follow the row filters, are discretised into 2 bins for the discrete tests when they look
    continuous, are shifted by +1 for "fz_nz" if they hold zeros (zeros mean "absent" there), lose zero-variance columns
    and are appended.  A normalizer that hands back a CSC table (the device front-end on a sparse count table) gets the meta block
    appended in CSC form as well: Int32 levels / Float32 values, a zero is an absent entry, the OTU part's stored zeros stay stored.
    norm (TSS_NORMS): the OTU columns take normalize(norm=...) -- a normalizer is expected to do the same -- and the meta variables
    the rules of the test_name the norm goes with: never shifted, discretised under "tss-nonzero-binned" only.
    n_bins, rank_method, disc_method (the binned modes, see normalize): the OTU columns take them -- a normalizer is expected to do the
    same -- and the meta variables do not: they go into 2 bins whatever n_bins is (preprocessing.jl:531-533).
    -> dict(data, header, meta_mask, row_mask)"""
    norm_check("normalize_with_meta", test_name, norm)
    bins_check("normalize_with_meta", test_name, n_bins, rank_method, disc_method)
    if make_onehot:
        md, mh = onehot(meta, meta_header)
    else:
        md, mh = np.asarray(meta, dtype=np.float64), list(meta_header or [""] * np.asarray(meta).shape[1])
    # normalizer: the OTU part on the device (engine.normalize_counts); the handful of meta columns stay here
    if normalizer is not None:
        data, row_mask, col_mask = normalizer(counts, test_name)
    else:
        data, row_mask, col_mask = normalize(counts, test_name, prec=prec, **({} if norm is None else {"norm": norm}),
                                             **bins_kw(n_bins, rank_method, disc_method))
    md, mh = prepare_meta_block(md, mh, test_name, row_mask)
    if _is_csc(data):
        *otu, rows = _csc_parts(data)
        out = _csc_hstack([tuple(otu), _csc_from_dense(md.astype(otu[2].dtype))], int(row_mask.sum()) if rows is None else rows)
    else:
        out = np.concatenate([data, md.astype(data.dtype)], axis=1)
    hdr = None
    if header is not None:
        hdr = [h for h, k in zip(header, col_mask) if k] + mh
    return dict(data=out, header=hdr, meta_header=mh, meta_mask=np.r_[np.zeros(out.shape[1] - md.shape[1], bool), np.ones(md.shape[1], bool)],
                row_mask=row_mask)


# The two norm modes of normalize_data that no test_name selects (preprocessing.jl:660-684), and the test_name a table so normalised
# is for: "tss" ("rows") is a continuous norm like clr_adapt, "tss-nonzero-binned" ("binned_nz_rows") a discrete one whose zeros are
# absences like binned_nz_clr.  The test_name is what the meta variables follow (prepare_meta_block): under "tss" they are neither
# discretised nor shifted, under "tss-nonzero-binned" continuous-looking ones go into 2 bins and none is shifted (:527-558).
TSS_NORMS = {"tss": "fz", "tss-nonzero-binned": "mi_nz"}


def norm_check(who, test_name, norm):
    """norm: None, or one of TSS_NORMS together with the test_name it goes with; anything else raises ValueError."""
    if norm is None:
        return
    if norm not in TSS_NORMS:
        raise ValueError("%s: unsupported norm %r (%s)" % (who, norm, ", ".join(map(repr, TSS_NORMS))))
    if test_name != TSS_NORMS[norm]:
        raise ValueError("%s: norm=%r goes with test_name=%r, got %r" % (who, norm, TSS_NORMS[norm], test_name))


def tss(data, prec=32):
    """rownorm! on a table converted to Float{prec} (preprocessing.jl:348-361 after check_convert_sparse): every value as a
    Float{prec}; s_i = the sum of sample i in that type, the columns added one after the other in ascending order from +0 (what
    Base's sum(X, dims=2) does; numpy's sum(axis=1) is pairwise and gives other bits); x / s_i, one IEEE division.  Only + and /:
    the device front-end returns the same bits."""
    X = np.asarray(data).astype(np.float32 if prec == 32 else np.float64)
    s = np.zeros(X.shape[0], dtype=X.dtype)
    for j in range(X.shape[1]):
        s = s + X[:, j]
    with np.errstate(under="ignore"):  # (a quotient below the smallest normal number is a subnormal, as on the device)
        return X / s[:, None]


def normalize(counts, test_name, prec=32, tie_anchor=False, norm=None, n_bins=3, rank_method="tied", disc_method="median"):
    """-> (data, row_mask, col_mask).  row/col masks refer to the input matrix.  tie_anchor: see adaptive_clr ("fz" only).
    norm (TSS_NORMS, with the test_name it goes with) replaces the test's transform, under the same filters:
      "tss"                 tss() of the filtered table                                               -> Float{prec} dense
      "tss-nonzero-binned"  the ranks, bins and column rule of "mi_nz" with the tss() value as the key; the non-zero mask is taken
                            before the division (a quotient may underflow to 0)                      -> Int32 {0,1,2}
    n_bins, rank_method ("tied" | "dense"), disc_method ("median" | "mean"): the options of the two binned modes ("mi_nz", and
    "tss-nonzero-binned"), see discretize_nz; levels 0 .. n_bins - 1, and a column is kept iff its non-zero entries show exactly
    n_bins - 1 distinct levels (preprocessing.jl:511-515).  Away from their defaults with any other mode: ValueError."""
    counts = np.asarray(counts)
    norm_check("normalize", test_name, norm)
    bins_check("normalize", test_name, n_bins, rank_method, disc_method)
    disc = dict(n_bins=n_bins, rank_method=rank_method, disc_method=disc_method)
    data, row_mask, col_mask = filter_by_variance(counts.astype(np.float64))
    cols = np.nonzero(col_mask)[0]
    if norm == "tss":
        return tss(data, prec), row_mask, col_mask
    if norm == "tss-nonzero-binned":
        nzm = data != 0
        c = tss(data, prec).astype(np.float64)  # (widening keeps order and ties)
        d = np.stack([discretize_nz(c[:, j], nzm[:, j], **disc) for j in range(c.shape[1])], axis=1)
        km = np.array([len(np.unique(d[d[:, j] != 0, j])) == n_bins - 1 for j in range(d.shape[1])])
        cm = np.zeros_like(col_mask)
        cm[cols[km]] = True
        return d[:, km].astype(np.int32), row_mask, cm
    if test_name == "fz":
        out, keep = adaptive_clr(data, tie_anchor=tie_anchor)
        rows = np.nonzero(row_mask)[0]
        row_mask = np.zeros_like(row_mask)
        row_mask[rows[keep]] = True
        return out.astype(np.float32 if prec == 32 else np.float64), row_mask, col_mask
    if test_name == "mi":
        b = np.sign(data).astype(np.int64)
        lv = np.array([len(np.unique(b[:, j])) for j in range(b.shape[1])])
        km = lv == 2
        cm = np.zeros_like(col_mask)
        cm[cols[km]] = True
        return b[:, km], row_mask, cm
    if test_name == "mi_nz":
        nzm = data != 0
        c = clr_nz(data)
        d = np.stack([discretize_nz(c[:, j], nzm[:, j], **disc) for j in range(c.shape[1])], axis=1)
        km = np.array([len(np.unique(d[d[:, j] != 0, j])) == n_bins - 1 for j in range(d.shape[1])])
        cm = np.zeros_like(col_mask)
        cm[cols[km]] = True
        return d[:, km], row_mask, cm
    if test_name == "fz_nz":  # clr_nz (preprocessing.jl:335-342): zeros stay zeros (= absences)
        out = clr_nz(data)
        return out.astype(np.float32 if prec == 32 else np.float64), row_mask, col_mask
    raise ValueError("unsupported test_name %r" % (test_name,))


# ---- several count tables of the same samples (preprocessing.jl:596-635 combine_data) ------------------------------------------
def _is_csc(t):
    """A sparse table: a scipy.sparse matrix, or a (colptr, rowval, nzval[, shape]) CSC triple with 0-based rows (what the device
    front-end hands back / engine.as_csc returns).  Tables here are outputs of a normalisation, so a tuple is never a dense table."""
    return isinstance(t, tuple) or (hasattr(t, "tocsc") and hasattr(t, "nnz"))


def _csc_parts(t):
    """-> (colptr, rowval, nzval, number of rows or None when a bare triple does not say)"""
    if isinstance(t, tuple):
        return t[0], t[1], t[2], (int(t[3][0]) if len(t) > 3 else None)
    m = t.tocsc()
    return m.indptr, m.indices, m.data, int(m.shape[0])


def _csc_take_rows(colptr, rowval, nzval, keep):
    """Rows `keep` (a mask over the table's rows) of a CSC triple, renumbered; O(nnz), stored zeros stay stored (a stored 0.0 of
    clr_nz is a present count)."""
    colptr, rowval, nzval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval), np.asarray(nzval)
    if keep.all():
        return colptr, rowval, nzval
    newrow = np.cumsum(keep) - 1  # the prefix sum over the mask renumbers the rows; ascending order inside a column survives
    sel = keep[rowval]
    upto = np.concatenate(([0], np.cumsum(sel, dtype=np.int64)))
    return upto[colptr], newrow[rowval[sel]], nzval[sel]


def _csc_take_cols(colptr, rowval, nzval, cols):
    """Columns `cols` (ascending indices) of a CSC triple, in that order; O(nnz), the entries of a column stay as they are stored
    (order, duplicates, stored zeros).  How a meta_mask splits a sparse table into its OTU block and its meta block."""
    colptr, rowval, nzval = np.asarray(colptr, dtype=np.int64), np.asarray(rowval), np.asarray(nzval)
    cols = np.asarray(cols, dtype=np.int64)
    lens = colptr[cols + 1] - colptr[cols]
    upto = np.concatenate(([0], np.cumsum(lens, dtype=np.int64)))
    src = np.repeat(colptr[cols] - upto[:-1], lens) + np.arange(upto[-1], dtype=np.int64)  # position k of the output reads src[k]
    return upto, rowval[src], nzval[src]


def _csc_to_dense(colptr, rowval, nzval, n):
    """A canonical CSC triple (no duplicates) as an n x q Float64 matrix, by a scatter of its own: for the few meta columns only (the
    reference's discretize_meta! densifies them, too) -- a table's OTU block never comes here."""
    q = len(colptr) - 1
    out = np.zeros((n, q), dtype=np.float64)
    out[np.asarray(rowval, dtype=np.int64), np.repeat(np.arange(q), np.diff(colptr))] = nzval
    return out


def _csc_from_dense(block):
    """A dense n x q block -> CSC triple of the block's dtype; a zero is an absent entry, rows ascending within a column."""
    cols, rows = np.nonzero(block.T)
    colptr = np.concatenate(([0], np.cumsum(np.bincount(cols, minlength=block.shape[1]), dtype=np.int64)))
    return colptr, rows, block[rows, cols]


def _csc_hstack(parts, n):
    """CSC triples over the same n rows, side by side -> scipy.sparse.csc_matrix assembled field by field (the constructor would
    re-check and could drop the stored 0.0f of clr_nz)."""
    import scipy.sparse as sp
    parts = [(np.asarray(c, dtype=np.int64), r, v) for c, r, v in parts]
    nnz = [int(c[-1]) for c, _, _ in parts]
    offs = np.concatenate(([0], np.cumsum(nnz)))
    colptr = np.concatenate([parts[0][0][:1]] + [c[1:] + o for (c, _, _), o in zip(parts, offs)])
    nzval = np.concatenate([v for _, _, v in parts])
    idx = np.int32 if max(n, len(colptr), int(offs[-1])) < 2**31 else np.int64  # (one index type, as scipy keeps it)
    out = sp.csc_matrix((n, len(colptr) - 1), dtype=nzval.dtype)
    out.indptr, out.indices, out.data = colptr.astype(idx), np.concatenate([r for _, r, _ in parts]).astype(idx), nzval
    return out


def combine_data(tables, headers, meta_masks, row_masks):
    """combine_data (preprocessing.jl:596-635): column-wise union of several normalised tables of the same n samples.
    tables[-1] is the main table (meta columns appended already), tables[:-1] the extra ones in the caller's order; row_masks[i] is
    the mask over the original n samples that the normalisation of table i kept (its rows, ascending); meta_masks[i] may be None
    (no meta variables: every extra table).  Every table is cut down to the samples all of them kept (a row gather), then the columns
    are laid out as the reference's pushfirst! leaves them: last extra, ..., first extra, main.  Nothing is filtered afterwards: a
    column that is constant on the common samples stays.  Dense arrays or CSC tables (_is_csc), never a mix; the CSC form gathers and
    stacks in O(nnz) and returns a scipy.sparse.csc_matrix assembled field by field (stored zeros are kept).
    -> (data, header, meta_mask, common row mask)"""
    k = len(tables)
    if k == 0 or not (len(headers) == len(meta_masks) == len(row_masks) == k):
        raise ValueError("combine_data: one header, meta mask and row mask per table")
    sparse = [_is_csc(t) for t in tables]
    if any(sparse) and not all(sparse):
        raise ValueError("combine_data: extra_data mixes sparse and dense tables; pass all of them in one form")
    masks = [np.asarray(m, dtype=bool) for m in row_masks]
    if any(m.shape != masks[0].shape for m in masks):
        raise ValueError("combine_data: extra_data tables are not over the same samples (row masks of %s entries)"
                         % sorted({int(m.size) for m in masks}))
    common = np.logical_and.reduce(masks)
    if not common.all():
        import warnings
        warnings.warn("%d samples had only zero counts in at least one data set and will not be used for inference"
                      % int((~common).sum()), stacklevel=2)
    parts, header, meta_mask = [], [], []
    for i in list(range(k - 2, -1, -1)) + [k - 1]:
        t, keep = tables[i], common[masks[i]]
        if sparse[i]:
            *t, have = _csc_parts(t)
            rows, cols = int(masks[i].sum()), len(t[0]) - 1
            if have is not None and have != rows:
                raise ValueError("combine_data: extra_data table %d has %d rows, its row mask keeps %d" % (i, have, rows))
            t = _csc_take_rows(*t, keep)
        else:
            t = np.asarray(t)
            rows, cols = int(masks[i].sum()), t.shape[1]
            if t.shape[0] != rows:
                raise ValueError("combine_data: extra_data table %d has %d rows, its row mask keeps %d" % (i, t.shape[0], rows))
            t = t if keep.all() else t[keep]
        if len(headers[i]) != cols:
            raise ValueError("combine_data: extra_data header %d names %d columns, its table has %d" % (i, len(headers[i]), cols))
        parts.append(t)
        header += list(headers[i])
        meta_mask.append(np.zeros(cols, bool) if meta_masks[i] is None else np.asarray(meta_masks[i], dtype=bool))
    meta_mask = np.concatenate(meta_mask)
    if not sparse[0]:
        return np.concatenate(parts, axis=1), header, meta_mask, common
    return _csc_hstack(parts, int(common.sum())), header, meta_mask, common
