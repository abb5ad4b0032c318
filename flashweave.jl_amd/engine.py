"""ctypes binding of include/flashweave_amd.h and the Python mirror of the reference's operator interface."""
import ctypes as C
import os
import sys
from collections import namedtuple

import numpy as np

from .preprocess import bins_check, bins_kw, norm_check

_HERE = os.path.dirname(os.path.abspath(__file__))
FW_MI, FW_MI_NZ, FW_FZ, FW_FZ_NZ = 0, 1, 2, 3
FW_MAX_K = 7
_KINDS = {"mi": FW_MI, "mi_nz": FW_MI_NZ, "fz": FW_FZ, "fz_nz": FW_FZ_NZ}
# The two transforms of the normalisation front-end that are no test kinds (normalize_data's norm_mode; preprocess.TSS_NORMS):
# the constants the fw_normalize_* entry points take as `kind`.
FW_NORM_TSS, FW_NORM_TSS_BINNED = 4, 5
_NORMS = {"tss": FW_NORM_TSS, "tss-nonzero-binned": FW_NORM_TSS_BINNED}
# The element type of what a fw_normalize_* entry point writes for a `kind` (out_f32 | out_i32; csrc/fw_norm_host.h: norm_kind).
NORM_OUT_DTYPE = {FW_FZ: np.float32, FW_FZ_NZ: np.float32, FW_NORM_TSS: np.float32, FW_MI: np.int32, FW_MI_NZ: np.int32,
                  FW_NORM_TSS_BINNED: np.int32}
# fw_norm_opts: the options of the binned kinds as the *_opts entry points take them (include/flashweave_amd.h)
FW_RANK = {"tied": 0, "dense": 1}
FW_DISC = {"median": 0, "mean": 1}
TSS_MIN, TSS_MAX = 2.0 ** -126, 2.0 ** 96  # positive real values a TSS norm takes: (float)x > 0, and fewer than 2^31 of them sum finitely

TestResult = namedtuple("TestResult", "stat pval df suff_power")  # src/types.jl:140-145


class FlashWeaveError(RuntimeError):
    """Raised for every non-zero ABI status (the reference throws Julia exceptions, e.g. learning.jl:72)."""

    def __init__(self, code, msg):
        super().__init__("[fw %d] %s" % (code, msg))
        self.code = code


class _Params(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n", C.c_int32), ("p", C.c_int32), ("device", C.c_int32),
                ("max_k", C.c_int32), ("hps", C.c_int32), ("fdr", C.c_int32), ("dense_rules", C.c_int32),
                ("n_obs_min", C.c_int64), ("max_tests", C.c_int64), ("alpha", C.c_double),
                ("recursive_pcor", C.c_int32), ("no_cor_mat", C.c_int32)]


class _NormOpts(C.Structure):  # fw_norm_opts
    _fields_ = [("n_bins", C.c_int32), ("rank_method", C.c_int32), ("disc_method", C.c_int32)]


class _TestResult(C.Structure):
    _fields_ = [("stat", C.c_double), ("pval", C.c_double), ("df", C.c_int32), ("suff_power", C.c_int32)]


class _SubsetsResult(C.Structure):
    _fields_ = [("stat", C.c_double), ("pval", C.c_double), ("df", C.c_int32), ("suff_power", C.c_int32),
                ("status", C.c_int32), ("n_zs", C.c_int32), ("zs", C.c_int32 * FW_MAX_K), ("reserved0", C.c_int32),
                ("num_tests", C.c_int64), ("frac", C.c_double)]


class _Rejection(C.Structure):  # fw_rejection
    _fields_ = [("target", C.c_int32), ("candidate", C.c_int32), ("n_zs", C.c_int32), ("zs", C.c_int32 * FW_MAX_K),
                ("df", C.c_int32), ("suff_power", C.c_int32), ("phase", C.c_int32), ("n_acc", C.c_int32),
                ("num_tests", C.c_int64), ("frac", C.c_double), ("stat", C.c_double), ("pval", C.c_double)]


REJECTION_DTYPE = np.dtype([("target", "<i4"), ("candidate", "<i4"), ("n_zs", "<i4"), ("zs", "<i4", (FW_MAX_K,)), ("df", "<i4"),
                            ("suff_power", "<i4"), ("phase", "<i4"), ("n_acc", "<i4"), ("num_tests", "<i8"), ("frac", "<f8"),
                            ("stat", "<f8"), ("pval", "<f8")])


def rejections_dict(records):
    """fw_rejection records -> {target: {candidate: (Zs, (stat, pval, df, suff_power), (num_tests, frac))}}, the shape of the
    reference's rejections(net_result) (Dict{T, RejDict}, types.jl:152) with 0-based ids."""
    out = {}
    cols = [records[f].tolist() for f in ("target", "candidate", "n_zs", "zs", "stat", "pval", "df", "suff_power", "num_tests", "frac")]
    for T, c, k, zs, stat, pval, df, pw, nt, frac in zip(*cols):  # (columns as Python lists first: 350 000 records in ~0.3 s)
        out.setdefault(T, {})[c] = (tuple(zs[:k]), (stat, pval, df, bool(pw)), (nt, frac))
    return out


class _Counters(C.Structure):
    _fields_ = [("level0_tests", C.c_int64), ("cond_tests_ref", C.c_int64), ("cond_tests_evaluated", C.c_int64),
                ("subsets_calls", C.c_int64), ("kernel_launches", C.c_int64), ("subsets_launches", C.c_int64), ("t_level0_s", C.c_double), ("t_level0_host_s", C.c_double),
                ("t_cond_s", C.c_double), ("t_dev_subsets_s", C.c_double), ("t_host_advance_s", C.c_double),
                ("t_host_build_s", C.c_double), ("t_host_launch_s", C.c_double), ("t_host_wait_s", C.c_double), ("t_host_merge_s", C.c_double),
                ("alg_bytes_subsets", C.c_double), ("gram_jobs", C.c_int64), ("gram_alg_bytes", C.c_double), ("gram_alg_flops", C.c_double),
                ("l0_mfma_flops", C.c_double), ("t_l0_mfma_s", C.c_double)]


def elim_mode(fast_elim=True, no_red_tests=True):
    """fw_learn_opts.elim_mode of the reference's keywords: 0 fast_elim; 1 fast_elim = false; 2 fast_elim = no_red_tests = false
    (no_red_tests has no effect with fast_elim = true, hiton.jl:388-390)."""
    return 0 if fast_elim else (1 if no_red_tests else 2)


class _LearnOpts(C.Structure):
    _fields_ = [("feed_forward", C.c_int32), ("round_size", C.c_int32), ("rank", C.c_int32),
                ("world_size", C.c_int32), ("max_targets", C.c_int32), ("elim_mode", C.c_int32)]


PREPARE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                         C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64))
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p)


class _DevExchange(C.Structure):  # fw_dev_exchange
    _fields_ = [("user", C.c_void_p), ("prepare", PREPARE_FN), ("exchange", EXCHANGE_FN)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                           C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64),
                           C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.POINTER(C.c_int32)),
                           C.POINTER(C.POINTER(C.c_double)), C.POINTER(C.POINTER(C.c_double)))

_LIB = None


def lib_path():
    # profiling builds of the same sources (e.g. -DFW_MI_TICKS, profiles/tools): honoured only under FW_KNOBS=1, like every FW_* knob
    alt = os.environ.get("FW_LIB_PATH") if os.environ.get("FW_KNOBS") == "1" else None
    return alt if alt else os.path.join(_HERE, "libflashweave_amd.so")


def load_library():
    """dlopen the in-tree library.  torch (if importable) is imported first so that a single HIP runtime
    (libamdhip64.so.7) ends up in the process."""
    global _LIB
    if _LIB is not None:
        return _LIB
    so = lib_path()
    if not os.path.exists(so):
        raise FlashWeaveError(-2, "libflashweave_amd.so is missing (run __graft_entry__.build()); there is no "
                                  "CPU fallback for the HIP path")
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(so)
    vp = C.c_void_p
    L.fw_abi_version.restype = C.c_int
    L.fw_params_default.argtypes = [C.POINTER(_Params), C.c_int32, C.c_int32, C.c_int32]
    L.fw_ctx_create.argtypes = [C.POINTER(_Params), C.POINTER(vp)]
    L.fw_ctx_destroy.argtypes = [vp]
    L.fw_last_error.restype = C.c_char_p
    L.fw_last_error.argtypes = [vp]
    L.fw_set_data_dense_f32.argtypes = [vp, vp]
    L.fw_set_data_csc_i32.argtypes = [vp, vp, vp, vp]
    L.fw_set_data_dense_i32.argtypes = [vp, vp]
    L.fw_get_levels.argtypes = [vp, vp, vp]
    L.fw_set_cor_mat.argtypes = [vp, vp]
    L.fw_compute_cor_mat.argtypes = [vp]
    L.fw_get_cor_mat.argtypes = [vp, vp]
    if hasattr(L, "fw_set_data_dense_f64"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        L.fw_set_data_dense_f64.argtypes = [vp, vp]
        L.fw_set_cor_mat_f64.argtypes = [vp, vp]
        L.fw_get_cor_mat_f64.argtypes = [vp, vp]
    L.fw_level0.argtypes = [vp, C.POINTER(C.c_int64)]
    L.fw_level0_get.argtypes = [vp, vp, vp, vp, vp]
    L.fw_set_row_views.argtypes = [vp, C.c_int32]
    L.fw_set_track_rejections.argtypes = [vp, C.c_int32]
    L.fw_rejections_count.argtypes = [vp, C.POINTER(C.c_int64)]
    L.fw_rejections_get.argtypes = [vp, vp]
    L.fw_normalize_counts.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32)]
    if hasattr(L, "fw_normalize_counts_csc"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        L.fw_normalize_counts_csc.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp, vp, vp, vp,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
        L.fw_set_data_csc_f32.argtypes = [vp, vp, vp, vp]
    if hasattr(L, "fw_normalize_abund"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        L.fw_normalize_abund.argtypes = L.fw_normalize_counts.argtypes
        L.fw_normalize_abund_csc.argtypes = L.fw_normalize_counts_csc.argtypes
    if hasattr(L, "fw_normalize_counts_opts"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        for name in ("fw_normalize_counts", "fw_normalize_counts_csc", "fw_normalize_abund", "fw_normalize_abund_csc"):
            getattr(L, name + "_opts").argtypes = getattr(L, name).argtypes + [C.POINTER(_NormOpts)]
    if hasattr(L, "fw_set_data_dense_i32_dev"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        L.fw_set_data_dense_i32_dev.argtypes = [vp, vp]
        L.fw_set_data_dense_f32_dev.argtypes = [vp, vp]
        L.fw_normalize_counts_dev.argtypes = L.fw_normalize_counts.argtypes + [C.POINTER(_NormOpts)]
        L.fw_normalize_abund_dev.argtypes = L.fw_normalize_counts_dev.argtypes
    if hasattr(L, "fw_set_data_csc_i32_dev"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        for name in ("fw_set_data_csc_i32_dev", "fw_set_data_csc_f32_dev", "fw_set_data_csc_f32_resident_dev"):
            getattr(L, name).argtypes = [vp, vp, vp, vp, C.c_int64]
        L.fw_normalize_counts_csc_dev.argtypes = ([C.c_int32] * 4 + [vp, vp, vp, C.c_int64, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                                     C.POINTER(C.c_int64), C.POINTER(_NormOpts)])
        L.fw_normalize_abund_csc_dev.argtypes = L.fw_normalize_counts_csc_dev.argtypes
    if hasattr(L, "fw_set_data_csc_f32_resident"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        L.fw_set_data_csc_f32_resident.argtypes = [vp, vp, vp, vp]
        L.fw_data_resident_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.fw_level0_sharded.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.POINTER(C.c_int64)]
    L.fw_level0_sharded_dev.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(_DevExchange), C.POINTER(C.c_int64)]
    L.fw_use_cor_buffer.argtypes = [vp, vp, C.c_int64]
    L.fw_compute_cor_mat_rows.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.fw_cor_mat_ready.argtypes = [vp]
    L.fw_test_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp]
    L.fw_test_subsets_batch.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp]
    L.fw_learn_network.argtypes = [vp, C.POINTER(_LearnOpts), vp, vp, C.POINTER(C.c_int64)]
    L.fw_learn_network_dev.argtypes = [vp, C.POINTER(_LearnOpts), C.POINTER(_DevExchange), C.POINTER(C.c_int64)]
    if hasattr(L, "fw_learn_neighbors"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        L.fw_learn_neighbors.argtypes = [vp, C.POINTER(_LearnOpts), vp, C.c_int32, C.POINTER(C.c_int64)]
    L.fw_network_get.argtypes = [vp, vp, vp, vp]
    L.fw_network_get_directed.argtypes = [vp, vp, vp, vp, vp]
    L.fw_get_counters.argtypes = [vp, C.POINTER(_Counters)]
    L.fw_reset_counters.argtypes = [vp]
    if hasattr(L, "fw_comm_init"):
        L.fw_comm_unique_id.argtypes = [vp]
        L.fw_comm_init.argtypes = [vp, vp, C.c_int32, C.c_int32]
        L.fw_comm_destroy.argtypes = [vp]
        L.fw_comm_stats.argtypes = [vp, vp, vp, vp, vp, vp]
        L.fw_level0_comm.argtypes = [vp, vp]
        L.fw_cor_mat_allgather_comm.argtypes = [vp, C.c_int64]
        L.fw_learn_network_comm.argtypes = [vp, vp, vp]
    if hasattr(L, "fw_rejections_allgather_dev"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        L.fw_rejections_allgather_dev.argtypes = [vp, C.POINTER(_DevExchange)]
        L.fw_rejections_allgather_comm.argtypes = [vp]
        L.fw_rejections_allgather_stats.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    if hasattr(L, "fw_selftest"):  # (absent from older builds loaded through FW_LIB_PATH for A/B profiling)
        L.fw_selftest.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]
    L.fw_effective_n_obs_min.restype = C.c_int64
    L.fw_effective_n_obs_min.argtypes = [vp]
    _LIB = L
    return L


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def is_sparse(data):
    """True for a scipy.sparse matrix / array (scipy is only imported when the object looks like one)."""
    if not (hasattr(data, "tocsc") and hasattr(data, "nnz")):
        return False
    import scipy.sparse as sp
    return bool(sp.issparse(data))


def is_device_tensor(who, data):
    """True for a torch.Tensor in GPU memory (device.type "cuda": what PyTorch-ROCm calls a HIP device) -- the table then stays on the
    device from here to the engine; False for anything else, a CPU tensor included (it keeps going through np.asarray).  A tensor of
    any other device type (meta, xla, ...) has no bytes this library could take: ValueError."""
    torch = sys.modules.get("torch")  # (a tensor exists only where torch has been imported: nothing is imported to ask)
    if torch is None or not isinstance(data, torch.Tensor) or data.device.type == "cpu":
        return False
    if data.device.type != "cuda":
        raise ValueError("%s: a torch.Tensor on a %r device is not supported: pass a tensor in GPU memory (device type \"cuda\") or "
                         "a CPU tensor" % (who, data.device.type))
    return True


def is_sparse_csc_tensor(data):
    """True for a torch.Tensor with layout torch.sparse_csc, on any device: the one sparse tensor form that is served (in GPU memory)."""
    torch = sys.modules.get("torch")
    return torch is not None and isinstance(data, torch.Tensor) and data.layout == torch.sparse_csc


def _dev_csc(who, t, device, dtype=None, numeric="biuf"):
    """A 2-D sparse CSC tensor in GPU memory taken apart into the three plain device tensors the *_csc_*_dev entry points borrow:
    -> (colptr int64 [p + 1], rowval int32 [nnz], nzval [nnz] of `dtype` (None: as it came), (n, p)), 0-based and contiguous; the
    conversions run on the device (rows that come as int64 cost a 4 B / entry int32 copy) and the producer's stream is drained.  Shape,
    numeric dtype and device index are checked as _dev_table checks them, and -- with torch ops, before any library call -- that the
    column pointers start at 0, end at the length of both other arrays and never step down: every column's range then lies inside
    the two arrays.  Nothing is made canonical: rows out of order, duplicates and stored zeros are the library's to refuse.
    Keep the three tensors alive over the call."""
    import torch
    if t.dim() != 2 or _tensor_np_kind(t) not in numeric:
        raise ValueError("%s: a device tensor must be a 2-D samples x variables table of a numeric dtype (got %d dimensions, %s)"
                         % (who, t.dim(), t.dtype))
    if t.device.index != device:
        raise ValueError("%s: the tensor lives on %s while device=%d: pass the device the table is on (or tensor.cpu())" % (who, t.device, device))
    t = t.detach()
    n, p = (int(v) for v in t.shape)
    ccol, rows, vals = t.ccol_indices(), t.row_indices(), t.values()
    if vals.dim() != 1 or n >= 2**31 or p >= 2**31:
        raise ValueError("%s: a sparse CSC tensor must hold one scalar per stored entry and fit the 32-bit row / column index" % who)
    if rows.dtype != torch.int32 and rows.numel() and not (0 <= int(rows.min()) and int(rows.max()) < 2**31):
        raise ValueError("%s: the sparse CSC tensor is not canonical: a row index lies outside 0 .. 2^31 - 1" % who)
    colptr, rowval = ccol.to(torch.int64).contiguous(), rows.to(torch.int32).contiguous()
    nzval = (vals if dtype is None else vals.to(dtype)).contiguous()
    nnz = int(rowval.numel())
    if (colptr.numel() != p + 1 or nzval.numel() != nnz or int(colptr[0]) != 0 or int(colptr[-1]) != nnz
            or bool((colptr[1:] < colptr[:-1]).any())):
        raise ValueError("%s: the sparse CSC tensor is not canonical: ccol_indices must run from 0 to the number of stored entries (%d) "
                         "without stepping down, over %d columns" % (who, nnz, p))
    torch.cuda.current_stream(t.device).synchronize()
    return colptr, rowval, nzval, (n, p)


def _dev_table(who, t, device, dtype, numeric="biuf"):
    """A 2-D GPU tensor as the *_dev entry points borrow it: `dtype`, column-major (strides (1, n): taken as it is, anything else
    through t.t().contiguous()), on GPU `device`; the conversions run on the device and the producer's stream is drained before the
    pointer is handed over.  -> the tensor to take data_ptr() of (keep it alive over the call)."""
    import torch
    if t.layout != torch.strided:
        raise ValueError("%s: a sparse torch tensor is not supported: scipy.sparse is the sparse interface, pass tensor.to_dense() "
                         "or a scipy matrix built from tensor.cpu() (of the sparse layouts only tensor.to_sparse_csc() is taken where "
                         "a sparse table is)" % who)
    kind = "b" if t.dtype == torch.bool else "f" if t.dtype.is_floating_point else "c" if t.dtype.is_complex else "i"
    if t.dim() != 2 or kind not in numeric:
        raise ValueError("%s: a device tensor must be a 2-D samples x variables table of a numeric dtype (got %d dimensions, %s)"
                         % (who, t.dim(), t.dtype))
    if t.device.index != device:
        raise ValueError("%s: the tensor lives on %s while device=%d: pass the device the table is on (or tensor.cpu())" % (who, t.device, device))
    n = t.shape[0]
    t = t.detach()
    if t.dtype != dtype:
        t = t.to(dtype)
    if t.stride() != (1, n):
        t = t.t().contiguous().t()
    torch.cuda.current_stream(t.device).synchronize()
    return t


def _tensor_np_kind(v):
    """numpy's dtype.kind of a torch tensor's elements, for the checks both array types share"""
    import torch
    return "b" if v.dtype == torch.bool else "f" if v.dtype.is_floating_point else "c" if v.dtype.is_complex else "i"


class CSC(namedtuple("CSC", "colptr rowval nzval shape")):
    """The canonical triple as_csc returns; handing it to as_csc / normalize_counts / Engine.set_data again costs nothing."""
    __slots__ = ()


def as_csc(data, dtype):
    """Any scipy.sparse matrix / array, or a (colptr, rowval, nzval, (n, p)) tuple with 0-based indices -> the canonical CSC
    triple (colptr int64, rowval int32, nzval dtype, (n, p)): duplicates summed, explicit zeros dropped, rows ascending within a
    column -- the triple scipy.sparse.csc_matrix(dense) gives.  With an integer dtype the values must be integral and lie in
    0 .. 2^31 - 1 (what the device front-end takes, as api._integral asks of a dense table), else ValueError.  Pure host code, O(nnz)."""
    dtype = np.dtype(dtype)
    if isinstance(data, CSC) and data.nzval.dtype == dtype:
        return data  # already canonical
    import scipy.sparse as sp
    if isinstance(data, CSC):
        data = tuple(data)
    if isinstance(data, tuple):
        if len(data) != 4:
            raise ValueError("as_csc: a tuple must be (colptr, rowval, nzval, (n, p))")
        m = sp.csc_matrix((np.asarray(data[2]), np.asarray(data[1]), np.asarray(data[0])), shape=tuple(int(v) for v in data[3]))
    elif sp.issparse(data):
        m = sp.csc_matrix(data)
    else:
        raise ValueError("as_csc: expected a scipy.sparse matrix or a (colptr, rowval, nzval, (n, p)) tuple, got %s" % type(data).__name__)
    if m.data.dtype.kind not in "iuf":
        raise ValueError("as_csc: values must be real numbers (got %s)" % m.data.dtype)
    # sums of duplicates in a type that cannot wrap before the range check
    m = m.astype(np.float64 if m.data.dtype.kind == "f" else np.int64 if m.data.dtype.kind == "i" else np.uint64, copy=True)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    v = m.data
    if dtype.kind in "iu":
        if v.size and v.dtype.kind == "f" and (not np.all(np.isfinite(v)) or np.any(v != np.floor(v))):
            raise ValueError("as_csc: non-integral values where integer counts are expected")
        if v.size and (v.min() < 0 or v.max() > np.iinfo(np.int32).max):
            raise ValueError("as_csc: counts must lie in 0 .. 2^31 - 1")
    n, p = m.shape
    if n >= 2**31 or p >= 2**31:
        raise ValueError("as_csc: the shape exceeds the 32-bit row / column index")
    return CSC(np.ascontiguousarray(m.indptr, dtype=np.int64), np.ascontiguousarray(m.indices, dtype=np.int32),
               np.ascontiguousarray(v, dtype=dtype), (int(n), int(p)))


def _front_end_kind(who, test_name, norm):
    """The `kind` a fw_normalize_* entry point is called with: the test kind, or the constant of a TSS norm (preprocess.norm_check
    says which test_name such a norm goes with)."""
    if norm is None:
        return _KINDS[test_name]
    norm_check(who, test_name, norm)
    return _NORMS[norm]


def tss_range_defect(values):
    """What keeps real values out of a TSS norm, as words for a refusal, or None: a positive value outside [2^-126, 2^96] (as a
    Float32 it could vanish, or the Float32 sum of a sample could overflow)."""
    if is_device_tensor("tss_range_defect", values):  # the same rule in torch ops on the device
        pos = values[values > 0] if _tensor_np_kind(values) == "f" else values[:0]
        if pos.numel() and (float(pos.min()) < TSS_MIN or float(pos.max()) > TSS_MAX):
            return "a positive value outside [2^-126, 2^96] (%r)" % float(pos.min() if float(pos.min()) < TSS_MIN else pos.max())
        return None
    v = np.asarray(values)
    if v.size and v.dtype.kind == "f":
        pos = v[v > 0]
        if pos.size and (pos.min() < TSS_MIN or pos.max() > TSS_MAX):
            return "a positive value outside [2^-126, 2^96] (%r)" % float(pos.min() if pos.min() < TSS_MIN else pos.max())
    return None


def _opts_arg(front_end, n_bins=3, rank_method="tied", disc_method="median"):
    """The last argument of an *_opts entry point -- the options as a fw_norm_opts, the defaults spelled out too -- or nothing for an
    entry point without options, which is never handed any."""
    if not (front_end.argtypes and front_end.argtypes[-1] is C.POINTER(_NormOpts)):
        assert not bins_kw(n_bins, rank_method, disc_method), "options need an *_opts entry point"
        return ()
    return (C.byref(_NormOpts(int(n_bins), FW_RANK[rank_method], FW_DISC[disc_method])),)


def _opts_front_end(L, who, name, bins):
    """The entry point `name`, or its *_opts sibling when any of the three options is away from its default (bins: bins_kw)."""
    if not bins:
        return getattr(L, name)
    if not hasattr(L, name + "_opts"):
        raise FlashWeaveError(-2, "%s: the loaded library has no %s_opts (an older build)" % (who, name))
    return getattr(L, name + "_opts")


def _normalize_csc(front_end, who, triple, test_name, device, norm=None, **bins):
    """fw_normalize_counts_csc / fw_normalize_abund_csc or their *_opts siblings (front_end) on the canonical triple
    -> (data, row_mask, col_mask)"""
    import scipy.sparse as sp
    L = load_library()
    colptr, rowval, nzval, (n, p) = triple
    if n <= 0 or p <= 0:
        raise ValueError("%s: counts must be a samples x OTUs matrix" % who)
    kind = _front_end_kind(who, test_name, norm)
    nnz = int(colptr[-1])
    rm, cm = np.zeros(n, np.uint8), np.zeros(p, np.uint8)
    no, po, nz = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    ocp, orow = np.zeros(p + 1, np.int64), np.zeros(max(nnz, 1), np.int32)
    of = np.zeros(n * p if kind == FW_FZ else max(nnz, 1), np.float32) if NORM_OUT_DTYPE[kind] is np.float32 else None
    oi = np.zeros(max(nnz, 1), np.int32) if NORM_OUT_DTYPE[kind] is np.int32 else None
    rc = front_end(device, kind, n, p, _ptr(colptr), _ptr(rowval), _ptr(nzval), _ptr(ocp), _ptr(orow), _ptr(oi), _ptr(of),
                   _ptr(rm), _ptr(cm), C.byref(no), C.byref(po), C.byref(nz), *_opts_arg(front_end, **bins))
    if rc != 0:
        raise FlashWeaveError(rc, L.fw_last_error(None).decode())
    if kind == FW_FZ:
        out = of[:no.value * po.value].reshape((no.value, po.value), order="F")
    else:  # (assembled field by field: the constructor would re-check and could drop the stored 0.0f of clr_nz)
        out = sp.csc_matrix((no.value, po.value), dtype=np.float32 if of is not None else np.int32)
        out.indptr, out.indices = ocp[:po.value + 1].astype(np.int32), orow[:nz.value].copy()  # (one index type, as scipy keeps it)
        out.data = (of if of is not None else oi)[:nz.value].copy()
    return out, rm.astype(bool), cm.astype(bool)


def _norm_kw(norm):
    """norm as a keyword for the next layer, only when one is given: a call without it is handed on as it always was."""
    return {} if norm is None else {"norm": norm}


def normalize_counts(counts, test_name, device=0, norm=None, n_bins=3, rank_method="tied", disc_method="median"):
    """Normalisation front-end on the device (fw_normalize_counts): -> (data, row_mask, col_mask) like preprocess.normalize,
    for every test_name ("fz": clr_adapt, "fz_nz": clr_nz, "mi": binary, "mi_nz": binned_nz_clr).
    A scipy.sparse count table (or what as_csc returned) takes fw_normalize_counts_csc and stays sparse: data is then a
    scipy.sparse.csc_matrix (Int32 for "mi" / "mi_nz", Float32 for "fz_nz", where a stored 0.0 is a present count whose clr_nz value
    is 0) and a dense array for "fz"; the values are the bits the dense table gives.
    norm: "tss" (with test_name "fz") or "tss-nonzero-binned" (with "mi_nz") replaces the test's transform by total-sum scaling in
    Float32 / by the binned ranks of its non-zero values, as preprocess.normalize(norm=...) computes them, bit for bit; a sparse table
    comes back sparse for both (Float32 / Int32).
    n_bins, rank_method ("tied" | "dense"), disc_method ("median" | "mean"): the options of the two binned modes ("mi_nz", and norm
    "tss-nonzero-binned"), as preprocess.normalize takes and computes them: Int32 levels 0 .. n_bins - 1.  Away from their defaults
    the call goes to fw_normalize_counts_opts / fw_normalize_counts_csc_opts; a value out of range, or an option given with a mode that
    does not bin, raises ValueError naming it before anything is loaded.
    A 2-D torch.Tensor in GPU memory (device.type "cuda", on GPU `device`) is borrowed where it is (fw_normalize_counts_dev): the
    checks above run as torch ops on the device, and data comes back as a tensor on that device -- an (n_out, p_out) view with
    strides (1, n_out) of the output buffer, the bits the numpy table gives; the masks are numpy.  normalize_abundances likewise
    (fw_normalize_abund_dev).  A CPU tensor is an array; any other device type raises ValueError.
    A 2-D sparse CSC tensor in GPU memory (layout torch.sparse_csc; torch.sparse_csc_tensor over a canonical scipy triple is one) is
    the sparse table of that path: its three arrays are borrowed (fw_normalize_counts_csc_dev / fw_normalize_abund_csc_dev), the value
    checks run on values(), and data comes back as a sparse CSC tensor over views of the output buffers (Int32 / Float32; a dense
    tensor for "fz"), the bits of the scipy call.  The tensor must be canonical already -- rows ascending in every column, no
    duplicates, no stored zeros: nothing is summed, dropped or sorted on the device, a defect is refused (FlashWeaveError naming the
    column).  Every other sparse layout (COO, CSR, BSR, BSC) raises ValueError."""
    if norm is not None:
        _front_end_kind("normalize_counts", test_name, norm)  # (an unknown or misplaced norm is refused before anything is loaded)
    bins_check("normalize_counts", test_name, n_bins, rank_method, disc_method)
    bins = bins_kw(n_bins, rank_method, disc_method)
    if is_device_tensor("normalize_counts", counts):
        if is_sparse_csc_tensor(counts):
            return _normalize_counts_csc_dev(counts, test_name, device, norm, bins)
        return _normalize_counts_dev(counts, test_name, device, norm, bins)
    L = load_library()
    if is_sparse(counts) or isinstance(counts, CSC):  # (any other tuple is a dense table, as before)
        return _normalize_csc(_opts_front_end(L, "normalize_counts", "fw_normalize_counts_csc", bins), "normalize_counts", as_csc(counts, np.int32),
                              test_name, device, **_norm_kw(norm), **bins)
    raw = np.asarray(counts)
    if raw.ndim != 2:
        raise ValueError("normalize_counts: counts must be a samples x OTUs matrix")
    if not np.issubdtype(raw.dtype, np.integer):  # a silent cast would truncate relative abundances / floats to zero
        if not np.all(np.isfinite(raw)) or np.any(raw != np.floor(raw)):
            raise TypeError("normalize_counts: the device front-end takes integer counts (got non-integral %s values)" % raw.dtype)
    if raw.size and (raw.min() < 0 or raw.max() > np.iinfo(np.int32).max):
        raise ValueError("normalize_counts: counts must lie in [0, 2^31 - 1]")
    return _normalize_dense(_opts_front_end(L, "normalize_counts", "fw_normalize_counts", bins), np.asfortranarray(raw.astype(np.int32)), test_name,
                            device, **_norm_kw(norm), **bins)


def _normalize_counts_dev(counts, test_name, device, norm, bins):
    """normalize_counts for a GPU tensor: the checks of the numpy path in torch ops on the device, then fw_normalize_counts_dev"""
    import torch
    who = "normalize_counts"
    x = _dev_table(who, counts, device, counts.dtype)  # (the refusals of shape, dtype and device first; the values as they came)
    if _tensor_np_kind(x) == "f":  # a silent cast would truncate relative abundances / floats to zero
        if not bool(torch.isfinite(x).all()) or bool((x != torch.floor(x)).any()):
            raise TypeError("normalize_counts: the device front-end takes integer counts (got non-integral %s values)" % x.dtype)
    if x.numel() and (float(x.min()) < 0 or float(x.max()) > np.iinfo(np.int32).max):
        raise ValueError("normalize_counts: counts must lie in [0, 2^31 - 1]")
    return _normalize_dense_dev("fw_normalize_counts_dev", who, _dev_table(who, x, device, torch.int32), test_name, device, norm, bins)


def _normalize_counts_csc_dev(counts, test_name, device, norm, bins):
    """normalize_counts for a sparse CSC tensor in GPU memory: the value checks of the dense device path on values(), in torch ops, then
    fw_normalize_counts_csc_dev on the borrowed triple"""
    import torch
    who = "normalize_counts"
    colptr, rowval, v, shape = _dev_csc(who, counts, device)  # (the refusals of shape, dtype, device and column pointers first)
    if _tensor_np_kind(v) == "f":  # a silent cast would truncate relative abundances / floats to zero
        if not bool(torch.isfinite(v).all()) or bool((v != torch.floor(v)).any()):
            raise TypeError("normalize_counts: the device front-end takes integer counts (got non-integral %s values)" % v.dtype)
    if v.numel() and (float(v.min()) < 0 or float(v.max()) > np.iinfo(np.int32).max):
        raise ValueError("normalize_counts: counts must lie in [0, 2^31 - 1]")
    return _normalize_csc_dev("fw_normalize_counts_csc_dev", who, (colptr, rowval, v.to(torch.int32), shape), test_name, device, norm, bins)


def _normalize_csc_dev(name, who, triple, test_name, device, norm, bins):
    """fw_normalize_counts_csc_dev / fw_normalize_abund_csc_dev on the three device tensors of _dev_csc -> (data, row_mask, col_mask):
    data a dense (n_out, p_out) view with strides (1, n_out) of the output buffer for "fz", else a sparse CSC tensor over views of the
    three output buffers (Int32 levels, Float32 values; no copy, no invariant check: the library wrote a canonical triple); the masks
    numpy"""
    import torch
    L = load_library()
    if not hasattr(L, name):
        raise FlashWeaveError(-2, "%s: the loaded library has no %s (an older build)" % (who, name))
    colptr, rowval, nzval, (n, p) = triple
    if n <= 0 or p <= 0:
        raise ValueError("%s: counts must be a samples x OTUs matrix" % who)
    kind = _front_end_kind(who, test_name, norm)
    nnz, dev = int(rowval.numel()), colptr.device
    rm, cm = np.zeros(n, np.uint8), np.zeros(p, np.uint8)
    no, po, nz = C.c_int32(0), C.c_int32(0), C.c_int64(0)
    ocp, orow = torch.empty(p + 1, dtype=torch.int64, device=dev), torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    out = torch.empty(n * p if kind == FW_FZ else max(nnz, 1), dtype=torch.float32 if NORM_OUT_DTYPE[kind] is np.float32 else torch.int32,
                      device=dev)
    torch.cuda.current_stream(dev).synchronize()
    vp = lambda t: C.c_void_p(t.data_ptr())
    of, oi = (vp(out), None) if out.dtype == torch.float32 else (None, vp(out))
    opts = C.byref(_NormOpts(int(bins.get("n_bins", 3)), FW_RANK[bins.get("rank_method", "tied")], FW_DISC[bins.get("disc_method", "median")])) if bins else None
    rc = getattr(L, name)(device, kind, n, p, vp(colptr), vp(rowval), vp(nzval), nnz, vp(ocp), vp(orow), oi, of, _ptr(rm), _ptr(cm),
                          C.byref(no), C.byref(po), C.byref(nz), opts)
    if rc != 0:
        raise FlashWeaveError(rc, L.fw_last_error(None).decode())
    if kind == FW_FZ:
        data = out[:no.value * po.value].view(po.value, no.value).t()
    else:
        data = torch.sparse_csc_tensor(ocp[:po.value + 1], orow[:nz.value], out[:nz.value], size=(no.value, po.value), check_invariants=False)
    return data, rm.astype(bool), cm.astype(bool)


def _normalize_dense_dev(name, who, x, test_name, device, norm, bins):
    """fw_normalize_counts_dev / fw_normalize_abund_dev on the column-major GPU tensor x -> (tensor, row_mask, col_mask): the tensor an
    (n_out, p_out) view with strides (1, n_out) of the output buffer on x's device, the masks numpy"""
    import torch
    L = load_library()
    if not hasattr(L, name):
        raise FlashWeaveError(-2, "%s: the loaded library has no %s (an older build)" % (who, name))
    n, p = x.shape
    if n <= 0 or p <= 0:
        raise ValueError("%s: counts must be a samples x OTUs matrix" % who)
    rm, cm = np.zeros(n, np.uint8), np.zeros(p, np.uint8)
    no, po = C.c_int32(0), C.c_int32(0)
    kind = _front_end_kind("normalize", test_name, norm)
    out = torch.empty(n * p, dtype=torch.float32 if NORM_OUT_DTYPE[kind] is np.float32 else torch.int32, device=x.device)
    torch.cuda.current_stream(x.device).synchronize()
    of, oi = (C.c_void_p(out.data_ptr()), None) if out.dtype == torch.float32 else (None, C.c_void_p(out.data_ptr()))
    opts = C.byref(_NormOpts(int(bins.get("n_bins", 3)), FW_RANK[bins.get("rank_method", "tied")], FW_DISC[bins.get("disc_method", "median")])) if bins else None
    rc = getattr(L, name)(device, kind, n, p, C.c_void_p(x.data_ptr()), of, oi, _ptr(rm), _ptr(cm), C.byref(no), C.byref(po), opts)
    if rc != 0:
        raise FlashWeaveError(rc, L.fw_last_error(None).decode())
    return out[:no.value * po.value].view(po.value, no.value).t(), rm.astype(bool), cm.astype(bool)


def _normalize_dense(front_end, x, test_name, device, norm=None, **bins):
    """fw_normalize_counts / fw_normalize_abund or their *_opts siblings (front_end) on the column-major table
    -> (data, row_mask, col_mask)"""
    L = load_library()
    n, p = x.shape
    rm, cm = np.zeros(n, np.uint8), np.zeros(p, np.uint8)
    no, po = C.c_int32(0), C.c_int32(0)
    kind = _front_end_kind("normalize", test_name, norm)
    of = np.zeros(n * p, np.float32) if NORM_OUT_DTYPE[kind] is np.float32 else None
    oi = np.zeros(n * p, np.int32) if NORM_OUT_DTYPE[kind] is np.int32 else None
    rc = front_end(device, kind, n, p, _ptr(x), _ptr(of), _ptr(oi), _ptr(rm), _ptr(cm), C.byref(no), C.byref(po), *_opts_arg(front_end, **bins))
    if rc != 0:
        raise FlashWeaveError(rc, L.fw_last_error(None).decode())
    out = (of if of is not None else oi)[:no.value * po.value].reshape((no.value, po.value), order="F")
    return out, rm.astype(bool), cm.astype(bool)


def abundance_defect(values):
    """What keeps real values from being abundances, as words for a refusal, or None: a NaN, an infinite or a negative value."""
    if is_device_tensor("abundance_defect", values):  # the same rule in torch ops on the device
        import torch
        kind = _tensor_np_kind(values)
        if values.numel() and kind == "f" and not bool(torch.isfinite(values).all()):
            return "a NaN or an infinite value"
        if values.numel() and kind in "if" and float(values.min()) < 0:
            return "a negative value"
        return None
    v = np.asarray(values)
    if v.size and v.dtype.kind == "f" and not np.all(np.isfinite(v)):
        return "a NaN or an infinite value"
    if v.size and v.dtype.kind in "if" and v.min() < 0:
        return "a negative value"
    return None


def normalize_abundances(table, test_name, device=0, norm=None, n_bins=3, rank_method="tied", disc_method="median"):
    """normalize_counts for a real-valued table -- relative abundances, percentages, coverage-normalised counts, counts beyond
    2^31 - 1 -- on the device (fw_normalize_abund, fw_normalize_abund_csc): -> (data, row_mask, col_mask) in the forms normalize_counts
    returns.  The values are taken as Float64 (a dense array of booleans, integers or floats is widened, Float32 exactly; a sparse
    table goes through as_csc(table, np.float64)); a table of integers gives the bits normalize_counts gives.  A NaN, an infinite or a
    negative value and a table that is not two-dimensional raise ValueError before any device call.
    norm: as for normalize_counts; every value is rounded to Float32 first, and a positive value outside [2^-126, 2^96] raises
    ValueError before any device call.
    n_bins, rank_method, disc_method: as for normalize_counts (fw_normalize_abund_opts / fw_normalize_abund_csc_opts)."""
    who = "normalize_abundances"
    if norm is not None:
        _front_end_kind(who, test_name, norm)
    bins_check(who, test_name, n_bins, rank_method, disc_method)
    bins = bins_kw(n_bins, rank_method, disc_method)
    sparse = is_sparse(table) or isinstance(table, CSC)
    on_gpu = is_device_tensor(who, table)
    dev_csc = on_gpu and is_sparse_csc_tensor(table)
    if dev_csc:  # (the checks below then run on values(), in torch ops)
        import torch
        dev_triple = _dev_csc(who, table, device, torch.float64)
        values = dev_triple[2]
    elif on_gpu:
        import torch
        values = _dev_table(who, table, device, torch.float64)
    elif sparse:
        triple = as_csc(table, np.float64)
        values = triple.nzval
    else:
        raw = np.asarray(table)
        if raw.ndim != 2 or raw.dtype.kind not in "biuf":
            raise ValueError("%s: the table must be a samples x OTUs matrix of real numbers" % who)
        values = np.asfortranarray(raw, dtype=np.float64)
    defect = abundance_defect(values)
    if defect:
        raise ValueError("%s: the table holds %s: abundances are finite and >= 0" % (who, defect))
    defect = tss_range_defect(values) if norm is not None else None
    if defect:
        raise ValueError("%s: norm=%r: the table holds %s" % (who, norm, defect))
    if dev_csc:
        return _normalize_csc_dev("fw_normalize_abund_csc_dev", who, dev_triple, test_name, device, norm, bins)
    if on_gpu:
        return _normalize_dense_dev("fw_normalize_abund_dev", who, values, test_name, device, norm, bins)
    L = load_library()
    if not hasattr(L, "fw_normalize_abund"):
        raise FlashWeaveError(-2, "%s: the loaded library has no fw_normalize_abund (an older build)" % who)
    if sparse:
        return _normalize_csc(_opts_front_end(L, who, "fw_normalize_abund_csc", bins), who, triple, test_name, device, **_norm_kw(norm), **bins)
    return _normalize_dense(_opts_front_end(L, who, "fw_normalize_abund", bins), values, test_name, device, **_norm_kw(norm), **bins)


class Engine:
    """One engine context on one GPU (replaces make_test_object, src/misc.jl:34-45).

    test_name: "mi" | "mi_nz" | "fz" (src/types.jl:64-72).  Keyword defaults are learn_network's
    (src/learning.jl:466-473).

    prec (learn_network's keyword): 32 (default) -- every continuous matrix handed in is cast to Float32, whatever its dtype; 64, "fz"
    only -- set_data / set_cor_mat convert to Float64 and the context runs in Float64 mode (include/flashweave_amd.h): cor() /
    cor_mat() return Float64, pcor_rec rounds in Float64.  The keyword decides, never the dtype of an array."""

    def __init__(self, test_name, n, p, max_k=3, alpha=0.01, hps=5, n_obs_min=-1, max_tests=10_000_000, FDR=True,
                 device=0, dense_rules=False, recursive_pcor=True, dense_cor=True, prec=32):
        if prec not in (32, 64):
            raise ValueError("Engine: prec must be 32 or 64 (got %r)" % (prec,))
        if prec == 64 and test_name != "fz":
            raise ValueError("Engine: prec=64 is served for test_name \"fz\" only (got %r)" % (test_name,))
        self.prec = prec
        self.L = load_library()
        self.test_name = test_name
        self.n, self.p = int(n), int(p)
        P = _Params()
        self.L.fw_params_default(C.byref(P), _KINDS[test_name], self.n, self.p)
        P.device, P.max_k, P.alpha, P.hps = device, max_k, alpha, hps
        P.n_obs_min, P.max_tests, P.fdr = n_obs_min, max_tests, int(FDR)
        P.recursive_pcor = int(bool(recursive_pcor))  # False: conditional fz tests stream the sample columns (no cor_mat, statfuns.jl:19-21)
        P.no_cor_mat = int(not dense_cor)  # dense_cor = False (learning.jl:42): no p x p matrix at all; needs recursive_pcor = False
        P.dense_rules = int(bool(dense_rules))  # Matrix (dense) table methods instead of the SparseMatrixCSC ones
        self.h = C.c_void_p()
        rc = self.L.fw_ctx_create(C.byref(P), C.byref(self.h))
        if rc != 0:
            raise FlashWeaveError(rc, self.L.fw_last_error(None).decode())
        self.max_k = max_k
        self.device = int(device)
        self._cb = None

    # -- plumbing ------------------------------------------------------------------------------------
    def _ck(self, rc):
        if rc != 0:
            raise FlashWeaveError(rc, self.L.fw_last_error(self.h).decode())

    def _need(self, symbol, what):
        # (an older build loaded through FW_LIB_PATH for A/B profiling may lack the newer entry points: refused by name)
        if not hasattr(self.L, symbol):
            raise FlashWeaveError(-5, "%s is not served by this build of libflashweave_amd.so (%s is missing from %s)" % (what, symbol, lib_path()))

    def close(self):
        if getattr(self, "h", None):
            self.L.fw_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data ----------------------------------------------------------------------------------------
    def set_data(self, data, csc_resident=False):
        """fz: dense Float32 n x p; fz_nz: the same, a scipy.sparse matrix or a (colptr, rowval, nzval) CSC triple with float
        values (fw_set_data_csc_f32: zeros = absences, nothing is densified on the host); mi / mi_nz: integer n x p (dense
        ndarray), a scipy.sparse matrix or a (colptr, rowval, nzval) CSC triple with 0-based rows.
        csc_resident=True (fz_nz with sparse input or a triple only, else ValueError): the data stays sparse on the device as well
        (fw_set_data_csc_f32_resident: plane + base + the values != 0 instead of the n x p matrix); results are the same bits.
        A 2-D torch.Tensor in GPU memory (device.type "cuda", on this engine's device) never leaves the device: it is converted
        there (float32 for fz / fz_nz, int32 for mi / mi_nz; column-major) and the resident layout is built from it on the device
        (fw_set_data_dense_f32_dev / fw_set_data_dense_i32_dev), the same bits as the upload of tensor.cpu().numpy().  Not served,
        ValueError: csc_resident=True, prec=64, a sparse tensor, a tensor of another GPU.  A CPU tensor goes through np.asarray.
        A 2-D sparse CSC tensor in GPU memory (layout torch.sparse_csc) is the sparse form of that path, for mi / mi_nz / fz_nz, and
        with csc_resident=True for fz_nz: its three arrays are borrowed where they lie (fw_set_data_csc_i32_dev,
        fw_set_data_csc_f32_dev, fw_set_data_csc_f32_resident_dev) and leave the resident bytes of the scipy upload.  It must be
        canonical already (nothing is summed, dropped or sorted on the device): unsorted, duplicate or out-of-range rows, a stored
        zero or a value above 61 in a level table raise FlashWeaveError with the host form's code, naming the column; for fz_nz a
        stored 0.0 is an absence.  "fz", prec=64 and a tensor of another GPU: ValueError.  Any other sparse layout: ValueError."""
        if is_device_tensor("Engine.set_data", data):
            if is_sparse_csc_tensor(data):
                return self._set_data_csc_dev(data, csc_resident)
            return self._set_data_dev(data, csc_resident)
        if csc_resident:
            if self.test_name != "fz_nz":
                raise ValueError("Engine.set_data: csc_resident=True is served for test_name \"fz_nz\" only (got %r)" % (self.test_name,))
            if not (is_sparse(data) or isinstance(data, tuple)):
                raise ValueError("Engine.set_data: csc_resident=True takes a scipy.sparse matrix or a (colptr, rowval, nzval) CSC triple, "
                                 "not a dense matrix")
            self._need("fw_set_data_csc_f32_resident", "csc_resident=True")
        if is_sparse(data) or isinstance(data, CSC):
            if self.test_name == "fz":
                raise ValueError("Engine.set_data: the plain \"fz\" test takes a dense matrix (sparse input is served for mi, mi_nz and fz_nz)")
            if self.prec == 64:
                raise ValueError("Engine.set_data: prec=64 takes a dense matrix")
            colptr, rowval, nzval, shape = as_csc(data, np.float32 if self.test_name == "fz_nz" else np.int32)
            assert shape == (self.n, self.p)
            data = (colptr, rowval, nzval)
        if self.test_name == "fz_nz" and isinstance(data, tuple):
            colptr, rowval, nzval = (np.ascontiguousarray(data[0], dtype=np.int64),
                                     np.ascontiguousarray(data[1], dtype=np.int32),
                                     np.ascontiguousarray(data[2], dtype=np.float32))
            assert colptr.shape == (self.p + 1,)
            upload = self.L.fw_set_data_csc_f32_resident if csc_resident else self.L.fw_set_data_csc_f32
            self._ck(upload(self.h, _ptr(colptr), _ptr(rowval), _ptr(nzval)))
        elif self.test_name in ("fz", "fz_nz"):
            d = np.asfortranarray(np.asarray(data, dtype=np.float64 if self.prec == 64 else np.float32))
            assert d.shape == (self.n, self.p)
            self._ck((self.L.fw_set_data_dense_f64 if self.prec == 64 else self.L.fw_set_data_dense_f32)(self.h, _ptr(d)))
        elif isinstance(data, tuple):
            colptr, rowval, nzval = (np.ascontiguousarray(data[0], dtype=np.int64),
                                     np.ascontiguousarray(data[1], dtype=np.int32),
                                     np.ascontiguousarray(data[2], dtype=np.int32))
            self._ck(self.L.fw_set_data_csc_i32(self.h, _ptr(colptr), _ptr(rowval), _ptr(nzval)))
        else:
            d = np.asfortranarray(np.asarray(data, dtype=np.int32))
            assert d.shape == (self.n, self.p)
            self._ck(self.L.fw_set_data_dense_i32(self.h, _ptr(d)))

    def _set_data_dev(self, t, csc_resident):
        import torch
        who = "Engine.set_data"
        if csc_resident:
            raise ValueError("Engine.set_data: csc_resident=True takes a scipy.sparse matrix or a CSC triple, not a device tensor")
        if self.prec == 64:
            raise ValueError("Engine.set_data: prec=64 is not served for a device tensor (Float64 mode uploads from the host): pass tensor.cpu()")
        self._need("fw_set_data_dense_i32_dev", "a device tensor")
        continuous = self.test_name in ("fz", "fz_nz")
        d = _dev_table(who, t, self.device, torch.float32 if continuous else torch.int32)
        assert tuple(d.shape) == (self.n, self.p)
        self._ck((self.L.fw_set_data_dense_f32_dev if continuous else self.L.fw_set_data_dense_i32_dev)(self.h, C.c_void_p(d.data_ptr())))

    def _set_data_csc_dev(self, t, csc_resident):
        import torch
        who = "Engine.set_data"
        if self.prec == 64:
            raise ValueError("Engine.set_data: prec=64 is not served for a device tensor (Float64 mode uploads from the host): pass tensor.cpu()")
        if self.test_name == "fz":
            raise ValueError("Engine.set_data: the plain \"fz\" test takes a dense matrix (sparse input is served for mi, mi_nz and fz_nz)")
        if csc_resident and self.test_name != "fz_nz":
            raise ValueError("Engine.set_data: csc_resident=True is served for test_name \"fz_nz\" only (got %r)" % (self.test_name,))
        continuous = self.test_name == "fz_nz"
        name = ("fw_set_data_csc_f32_resident_dev" if csc_resident else "fw_set_data_csc_f32_dev") if continuous else "fw_set_data_csc_i32_dev"
        self._need(name, "a sparse CSC device tensor")
        colptr, rowval, v, shape = _dev_csc(who, t, self.device, torch.float32 if continuous else None)
        if not continuous:  # (what as_csc asks of a level table, in torch ops: a cast must not wrap or truncate)
            if _tensor_np_kind(v) == "f" and not (bool(torch.isfinite(v).all()) and bool((v == torch.floor(v)).all())):
                raise ValueError("Engine.set_data: non-integral values where integer levels are expected")
            if v.numel() and (float(v.min()) < 0 or float(v.max()) > np.iinfo(np.int32).max):
                raise ValueError("Engine.set_data: levels must lie in 0 .. 2^31 - 1")
            if v.dtype != torch.int32:  # (queued on torch's stream after _dev_csc drained it: the library reads on a stream of its own)
                v = v.to(torch.int32)
                torch.cuda.current_stream(v.device).synchronize()
        assert shape == (self.n, self.p)
        self._ck(getattr(self.L, name)(self.h, C.c_void_p(colptr.data_ptr()), C.c_void_p(rowval.data_ptr()), C.c_void_p(v.data_ptr()),
                                       int(rowval.numel())))

    def data_resident_bytes(self):
        """fz_nz: bytes of device memory the context holds for the data (fw_data_resident_bytes) -- 4 n p + 8 p W dense-resident,
        12 p W + 4 nnz' CSC-resident (W = ceil(n / 64), nnz' = values != 0)."""
        self._need("fw_data_resident_bytes", "data_resident_bytes()")
        b = C.c_int64(0)
        self._ck(self.L.fw_data_resident_bytes(self.h, C.byref(b)))
        return b.value

    def set_cor_mat(self, cor_mat):
        cm = np.asfortranarray(np.asarray(cor_mat, dtype=np.float64 if self.prec == 64 else np.float32))
        assert cm.shape == (self.p, self.p)
        self._ck((self.L.fw_set_cor_mat_f64 if self.prec == 64 else self.L.fw_set_cor_mat)(self.h, _ptr(cm)))

    def cor(self):
        """cor(data_dense) -> Float32 p x p (Float64 with prec=64), on the MFMA units (src/learning.jl:44)."""
        self._ck(self.L.fw_compute_cor_mat(self.h))
        return self.cor_mat()

    def compute_cor(self):
        """Device-only form of cor(): the matrix stays resident, nothing is copied back."""
        self._ck(self.L.fw_compute_cor_mat(self.h))

    def cor_mat(self):
        if self.prec == 64:
            out = np.zeros((self.p, self.p), dtype=np.float64, order="F")
            self._ck(self.L.fw_get_cor_mat_f64(self.h, _ptr(out)))
            return out
        out = np.zeros((self.p, self.p), dtype=np.float32, order="F")
        self._ck(self.L.fw_get_cor_mat(self.h, _ptr(out)))
        return out

    def set_row_views(self, on=True):
        """mi_nz + dense_rules: test_subsets on the (T, candidate) row views hiton.jl uses (include/flashweave_amd.h)."""
        self._ck(self.L.fw_set_row_views(self.h, int(bool(on))))

    def levels(self):
        lv, mv = np.zeros(self.p, np.int32), np.zeros(self.p, np.int32)
        self._ck(self.L.fw_get_levels(self.h, _ptr(lv), _ptr(mv)))
        return lv, mv

    @property
    def n_obs_min(self):
        return int(self.L.fw_effective_n_obs_min(self.h))

    # -- level 0 -------------------------------------------------------------------------------------
    def level0(self, rank=0, world_size=1, allgather=None):
        """Runs level 0 and keeps the neighbour lists in the context (no copy to Python); returns the entry count.
        world_size > 1: this rank screens its share of the pair tiles (discrete kinds) and the significant pairs are
        exchanged through `allgather` (flashweave.jl_amd/dist.py)."""
        nnz = C.c_int64(0)
        if world_size > 1:
            cb = ALLGATHER_FN(allgather)
            self._cb0 = cb
            self._ck(self.L.fw_level0_sharded(self.h, rank, world_size, C.cast(cb, C.c_void_p), None, C.byref(nnz)))
        else:
            self._ck(self.L.fw_level0(self.h, C.byref(nnz)))
        return nnz.value

    def level0_dev(self, rank, world_size, exchange):
        """Level 0 of a target-sharded run with the exchange kept in device memory (fw_level0_sharded_dev): `exchange` is a
        (prepare, exchange) pair of Python callables (dist.make_dev_exchange)."""
        nnz = C.c_int64(0)
        x = _DevExchange(None, PREPARE_FN(exchange[0]), EXCHANGE_FN(exchange[1]))
        self._xdev = x
        self._ck(self.L.fw_level0_sharded_dev(self.h, rank, world_size, C.byref(x), C.byref(nnz)))
        return nnz.value

    # -- library-side collectives (fw_comm_*: RCCL on a communicator the library owns) -------------------
    @staticmethod
    def comm_unique_id():
        """Rank 0: the 128-byte rendezvous id (ncclGetUniqueId); ship it to every rank, then comm_init everywhere."""
        L = load_library()
        buf = (C.c_uint8 * 128)()
        rc = L.fw_comm_unique_id(buf)
        if rc:
            raise FlashWeaveError(rc, (L.fw_last_error(None) or b"").decode())
        return bytes(buf)

    def comm_init(self, id128, rank, world_size):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(id128))
        self._ck(self.L.fw_comm_init(self.h, buf, int(rank), int(world_size)))

    def comm_destroy(self):
        self._ck(self.L.fw_comm_destroy(self.h))

    def comm_stats(self):
        a, b, c_, d = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        s_ = C.c_double(0)
        self._ck(self.L.fw_comm_stats(self.h, C.byref(a), C.byref(b), C.byref(c_), C.byref(d), C.byref(s_)))
        return dict(calls=a.value, collectives=b.value, entries=c_.value, bytes=d.value, seconds=s_.value)

    def level0_comm(self):
        """fw_level0_comm: level 0 with this rank's share of the pair tiles (discrete kinds), significant pairs all-gathered by the library."""
        nnz = C.c_int64(0)
        self._ck(self.L.fw_level0_comm(self.h, C.byref(nnz)))
        return nnz.value

    def cor_allgather_comm(self, rows_per_rank):
        self._ck(self.L.fw_cor_mat_allgather_comm(self.h, int(rows_per_rank)))

    def lgl_comm(self, feed_forward=True, round_size=1, max_targets=0, edge_dict=True, fast_elim=True, no_red_tests=True,
                 track_rejections=False):
        """fw_learn_network_comm: LGL of a target-sharded run, the per-round exchange issued by the library (rank / world_size are the
        communicator's).  fast_elim / no_red_tests / track_rejections: as in lgl (every rank gets the rejections of its own targets)."""
        self._set_track(track_rejections)
        opts = _LearnOpts(int(feed_forward), int(round_size), 0, 1, int(max_targets), elim_mode(fast_elim, no_red_tests))
        ne = C.c_int64(0)
        self._ck(self.L.fw_learn_network_comm(self.h, C.byref(opts), C.byref(ne)))
        return self._network(ne.value, edge_dict, track_rejections)

    # -- row-block sharding of cor() ------------------------------------------------------------------
    def use_cor_buffer(self, device_ptr, capacity_floats):
        """Keep the p x p matrix in caller-owned device memory (a torch tensor's data_ptr()): fw_use_cor_buffer."""
        self._ck(self.L.fw_use_cor_buffer(self.h, C.c_void_p(device_ptr), int(capacity_floats)))

    def compute_cor_rows(self, rank, world_size):
        """This rank's row block of the matrix -> (row0, rows_per_rank); gather the blocks, then cor_ready()."""
        r0, rp = C.c_int64(0), C.c_int64(0)
        self._ck(self.L.fw_compute_cor_mat_rows(self.h, rank, world_size, C.byref(r0), C.byref(rp)))
        return r0.value, rp.value

    def cor_ready(self):
        self._ck(self.L.fw_cor_mat_ready(self.h))

    def pw_univar_neighbors(self):
        """pw_univar_neighbors (src/tests.jl:436-532) -> CSR dict(off, idx, stat, pval)."""
        nnz = C.c_int64(0)
        self._ck(self.L.fw_level0(self.h, C.byref(nnz)))
        return self.pw_univar_neighbors_get()

    def pw_univar_neighbors_get(self):
        """The neighbour lists of the last level-0 run (fw_level0_get) -> CSR dict(off, idx, stat, pval)."""
        off = np.zeros(self.p + 1, np.int64)
        self._ck(self.L.fw_level0_get(self.h, _ptr(off), None, None, None))
        nnz = C.c_int64(int(off[-1]))
        k = max(nnz.value, 1)
        idx, stat, pv = np.zeros(k, np.int32), np.zeros(k, np.float64), np.zeros(k, np.float64)
        self._ck(self.L.fw_level0_get(self.h, _ptr(off), _ptr(idx), _ptr(stat), _ptr(pv)))
        return dict(off=off, idx=idx[:nnz.value], stat=stat[:nnz.value], pval=pv[:nnz.value])

    # -- single tests --------------------------------------------------------------------------------
    def test_batch(self, X, Y, Zs_list):
        """Batch of test(X, Y, Zs, ...) (src/tests.jl:28,108,184,250)."""
        m = len(X)
        Xa, Ya = np.asarray(X, np.int32), np.asarray(Y, np.int32)
        zoff = np.zeros(m + 1, np.int64)
        for i, z in enumerate(Zs_list):
            zoff[i + 1] = zoff[i] + len(z)
        zflat = np.array([v for z in Zs_list for v in z] or [0], dtype=np.int32)
        out = (_TestResult * m)()
        self._ck(self.L.fw_test_batch(self.h, m, _ptr(Xa), _ptr(Ya), _ptr(zoff), _ptr(zflat), out))
        return [TestResult(o.stat, o.pval, o.df, bool(o.suff_power)) for o in out]

    def test(self, X, Y, Zs=()):
        return self.test_batch([X], [Y], [tuple(Zs)])[0]

    def test_subsets_batch(self, T, cand, accepted_list):
        """Batch of test_subsets(T, candidate, accepted, ...) (src/tests.jl:281-346)."""
        m = len(T)
        Ta, Ca = np.asarray(T, np.int32), np.asarray(cand, np.int32)
        off = np.zeros(m + 1, np.int64)
        for i, a in enumerate(accepted_list):
            off[i + 1] = off[i] + len(a)
        flat = np.array([v for a in accepted_list for v in a] or [0], dtype=np.int32)
        out = (_SubsetsResult * m)()
        self._ck(self.L.fw_test_subsets_batch(self.h, m, _ptr(Ta), _ptr(Ca), _ptr(off), _ptr(flat), out))
        return [dict(status=o.status, stat=o.stat, pval=o.pval, df=o.df, suff_power=bool(o.suff_power),
                     Zs=tuple(o.zs[:o.n_zs]), num_tests=o.num_tests, frac=o.frac) for o in out]

    def test_subsets(self, T, cand, accepted):
        return self.test_subsets_batch([T], [cand], [list(accepted)])[0]

    def selftest(self, which=1, cases=1 << 28, seed=1):
        """fw_selftest: device-side bit comparison of a hand-written arithmetic sequence with the compiler's (1 = Float64 division)."""
        bad = C.c_uint64(0)
        self._ck(self.L.fw_selftest(self.h, which, cases, seed, C.byref(bad)))
        return int(bad.value)

    # -- LGL -----------------------------------------------------------------------------------------
    def lgl(self, feed_forward=True, round_size=1, rank=0, world_size=1, max_targets=0, allgather=None, edge_dict=True, dev_exchange=None,
            fast_elim=True, no_red_tests=True, track_rejections=False):
        """LGL minus normalisation (src/learning.jl:203-279).  Returns dict(edges={(i,j): w}, directed=CSR);
        edge_dict=False leaves the edges as the three arrays fw_network_get fills (edge_src, edge_dst, edge_weight) and
        skips the Python dictionary (48 000 tuples cost ~8 ms at cfg3).
        fast_elim=False: exact HITON-PC elimination (hiton.jl:67-70: a rejected member stays in the conditioning pool);
        no_red_tests=False (with fast_elim=False only): PC keeps the elimination-phase statistics (hiton.jl:388-390).
        track_rejections=True (learning.jl:446): the result also holds "rejections" = {target: {candidate: (Zs, (stat, pval, df,
        suff_power), (num_tests, frac))}} -- for every candidate a conditional test removed, the first non-significant test in the
        reference's order -- and "rejection_records", the same as a structured array (REJECTION_DTYPE, with the phase and the length
        of the accepted list; ascending target, candidate); edge_dict=False returns the array only.  The network is the same bytes
        either way."""
        self._set_track(track_rejections)
        opts = _LearnOpts(int(feed_forward), int(round_size), int(rank), int(world_size), int(max_targets), elim_mode(fast_elim, no_red_tests))
        ne = C.c_int64(0)
        cb = None
        if allgather is not None:
            cb = ALLGATHER_FN(allgather)
            self._cb = cb
        if dev_exchange is not None:  # (prepare, exchange) of dist.make_dev_exchange: the library packs / unpacks, Python runs the collective
            x = _DevExchange(None, PREPARE_FN(dev_exchange[0]), EXCHANGE_FN(dev_exchange[1]))
            self._xdev_lgl = x
            self._ck(self.L.fw_learn_network_dev(self.h, C.byref(opts), C.byref(x), C.byref(ne)))
        else:
            self._ck(self.L.fw_learn_network(self.h, C.byref(opts), C.cast(cb, C.c_void_p) if cb else None, None, C.byref(ne)))
        return self._network(ne.value, edge_dict, track_rejections)

    def neighbors(self, targets, round_size=0, edge_dict=True, fast_elim=True, no_red_tests=True, track_rejections=False):
        """fw_learn_neighbors: si_HITON_PC(T, data; ...) (src/hiton.jl:402-409) for a list of targets -- level 0 over all pairs (if it
        has not run), then HITON-PC for the listed variables only, each on its own (no feed-forward).  targets: distinct variable ids
        in 0 .. p-1, in any order.  Returns what lgl returns: a listed target's directed row is its row of lgl(feed_forward=False), to
        the bit, the rows of the other variables are empty, and the edges are make_symmetric_graph of those rows alone (an edge to an
        unlisted variable has one direction only); with track_rejections the log holds the listed targets' records.  round_size only
        batches the work.  The context keeps level 0 and the Pearson matrix: it can be asked again, and lgl can follow."""
        self._need("fw_learn_neighbors", "neighbors()")
        t = np.asarray(targets)
        t = t.astype(np.int32) if (t.ndim == 1 and t.size == 0) else t  # (an empty list: the library refuses it by name)
        if t.ndim != 1 or t.dtype.kind not in "iu":
            raise ValueError("neighbors: targets must be a list of variable ids (integers), got %s" % (t.dtype if t.ndim == 1 else "%d dimensions" % t.ndim))
        if t.size and (t.min() < -2**31 or t.max() >= 2**31):
            raise ValueError("neighbors: targets holds an id outside the Int32 range")
        t = np.ascontiguousarray(t, dtype=np.int32)
        self._set_track(track_rejections)
        opts = _LearnOpts(0, int(round_size), 0, 1, 0, elim_mode(fast_elim, no_red_tests))
        ne = C.c_int64(0)
        self._ck(self.L.fw_learn_neighbors(self.h, C.byref(opts), _ptr(t), int(t.size), C.byref(ne)))
        return self._network(ne.value, edge_dict, track_rejections)

    def _set_track(self, on):
        if bool(on) != getattr(self, "_track", False):  # (the switch of the context is only touched when it changes)
            self._ck(self.L.fw_set_track_rejections(self.h, int(bool(on))))
            self._track = bool(on)

    def rejection_records(self):
        """The rejection log of the last tracked lgl as a structured array (fw_rejections_count / fw_rejections_get)."""
        n = C.c_int64(0)
        self._ck(self.L.fw_rejections_count(self.h, C.byref(n)))
        rec = np.zeros(max(n.value, 1), REJECTION_DTYPE)
        self._ck(self.L.fw_rejections_get(self.h, _ptr(rec)))
        return rec[:n.value]

    def gather_rejections(self, dev_exchange):
        """fw_rejections_allgather_dev: COLLECTIVE -- every rank of a target-sharded run calls it once after a tracked lgl; afterwards
        rejection_records() is the log of all targets on every rank, the bytes of a one-rank log.  dev_exchange: the (prepare, exchange)
        pair lgl took (dist.make_dev_exchange).  A second call is a no-op.  -> dict(packed_host, packed_dev, received): records this
        rank sent that the host job pool / the device paths had written, and records of other ranks placed here."""
        self._need("fw_rejections_allgather_dev", "gather_rejections()")
        x = _DevExchange(None, PREPARE_FN(dev_exchange[0]), EXCHANGE_FN(dev_exchange[1]))
        self._xdev_rej = x
        self._ck(self.L.fw_rejections_allgather_dev(self.h, C.byref(x)))
        return self._gather_stats()

    def gather_rejections_comm(self):
        """fw_rejections_allgather_comm: gather_rejections on the library's own communicator (comm_init), after a tracked lgl_comm."""
        self._need("fw_rejections_allgather_comm", "gather_rejections_comm()")
        self._ck(self.L.fw_rejections_allgather_comm(self.h))
        return self._gather_stats()

    def _gather_stats(self):
        a, b, c_ = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._ck(self.L.fw_rejections_allgather_stats(self.h, C.byref(a), C.byref(b), C.byref(c_)))
        return dict(packed_host=a.value, packed_dev=b.value, received=c_.value)

    def _network(self, n_edges, edge_dict, track_rejections=False):
        ne = C.c_int64(n_edges)
        k = max(ne.value, 1)
        src, dst, w = np.zeros(k, np.int32), np.zeros(k, np.int32), np.zeros(k, np.float64)
        self._ck(self.L.fw_network_get(self.h, _ptr(src), _ptr(dst), _ptr(w)))
        off = np.zeros(self.p + 1, np.int64)
        self._ck(self.L.fw_network_get_directed(self.h, _ptr(off), None, None, None))
        kk = max(int(off[-1]), 1)
        idx, pw, pp = np.zeros(kk, np.int32), np.zeros(kk, np.float64), np.zeros(kk, np.float64)
        self._ck(self.L.fw_network_get_directed(self.h, _ptr(off), _ptr(idx), _ptr(pw), _ptr(pp)))
        m = ne.value
        out = dict(edge_src=src[:m], edge_dst=dst[:m], edge_weight=w[:m], pc_off=off, pc_idx=idx[:off[-1]],
                   pc_weight=pw[:off[-1]], pc_pval=pp[:off[-1]])
        if edge_dict:
            out["edges"] = dict(zip(zip(src[:m].tolist(), dst[:m].tolist()), w[:m].tolist()))  # python ints / floats
        out["rejections"] = {}
        if track_rejections:
            out["rejection_records"] = self.rejection_records()
            if edge_dict:  # (edge_dict=False skips this dictionary as well: rejections_dict(net["rejection_records"]) builds it later)
                out["rejections"] = rejections_dict(out["rejection_records"])
        return out

    def counters(self):
        cn = _Counters()
        self._ck(self.L.fw_get_counters(self.h, C.byref(cn)))
        return {f: getattr(cn, f) for f, _ in _Counters._fields_}

    def reset_counters(self):
        self._ck(self.L.fw_reset_counters(self.h))
