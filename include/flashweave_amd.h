/*
 * flashweave_amd.h -- C ABI of the MI355X-native conditional-independence engine for FlashWeave.
 *
 * This is the drop-in boundary for ONE path of the reference (FlashWeave.jl, /root/reference): the
 * per-pair CI test batch + the level-0 all-pairs stage (src/tests.jl, src/contingency.jl, src/statfuns.jl).
 * The reference has no FFI for it; the seam is Julia multiple dispatch on `test_obj::AbstractTest`
 * (src/types.jl:57-59).  Each entry point below names the reference call edge it replaces, and
 * INTEGRATION.md shows the `ccall` methods a maintainer would add for a `GpuTest <: AbstractTest`.
 *
 * Conventions
 *   - plain C, no C++/torch types; all buffers are caller-owned host memory unless stated otherwise;
 *     the context owns every device allocation.
 *   - variable indices are 0-based on this ABI (the Julia shim subtracts 1).
 *   - data is n samples (rows) x p variables (columns), column-major, exactly as Julia holds it.
 *   - every function returns FW_OK (0) or a negative error code; fw_last_error() gives the message.
 *     Invalid input never aborts the process (reference: error()/@assert, e.g. src/learning.jl:72).
 *   - a context is used by one host thread at a time; calls are blocking; one context per GPU.
 *   - there is NO CPU fallback: if no gfx950 device is usable, fw_ctx_create fails with FW_ERR_DEVICE.
 */
#ifndef FLASHWEAVE_AMD_H
#define FLASHWEAVE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FW_ABI_VERSION 6 /* 2: fw_params.recursive_pcor, fw_level0_sharded; 3: device-resident exchange (fw_dev_exchange), sharded cor; 4: fw_params.no_cor_mat; 5: fw_selftest, fw_counters.gram_*, fw_comm_* (library-side RCCL); 6: FW_MAX_K 5 -> 7 (fw_subsets_result.zs grows) */

/* test kinds: src/types.jl:61-72 (test_name "mi" / "mi_nz" / "fz") */
#define FW_MI 0
#define FW_MI_NZ 1
#define FW_FZ 2
#define FW_FZ_NZ 3 /* "fz_nz": FlashWeaveHE-S, zero-ignoring Fisher-z tests */
/* Not test kinds: two further transforms of the normalisation front-end, taken as `kind` by the four fw_normalize_* entry points
 * only (fw_params.kind refuses them).  Additive: the ABI version stays. */
#define FW_NORM_TSS 4        /* norm_mode "tss": total-sum scaling in Float32 */
#define FW_NORM_TSS_BINNED 5 /* norm_mode "tss-nonzero-binned": the tied ranks of the non-zero TSS values in two bins */

#define FW_OK 0
#define FW_ERR_ARG (-1)     /* invalid argument */
#define FW_ERR_DEVICE (-2)  /* no usable gfx950 device / HIP runtime error */
#define FW_ERR_STATE (-3)   /* call order violated (e.g. level-0 before data upload) */
#define FW_ERR_NOBS (-4)    /* n_obs_min exceeds the number of samples (src/learning.jl:66-73) */
#define FW_ERR_LIMIT (-5)   /* a documented capacity limit was exceeded (max_k, table size) */
#define FW_ERR_NOMEM (-6)

#define FW_MAX_K 7 /* largest conditioning-set size (tests.jl:311-343 has no cap): up to 5 on the table / persistent kernels, 6 and 7 (ABI 6) on
                      general-form kernels through the host job pool; not with recursive_pcor = 0 */

typedef struct fw_ctx fw_ctx;

/* Engine parameters; defaults follow learn_network / LGL (src/learning.jl:203-214,466-473). */
typedef struct fw_params {
    int32_t kind;      /* FW_MI / FW_MI_NZ / FW_FZ / FW_FZ_NZ */
    int32_t n;         /* samples (rows) */
    int32_t p;         /* variables (columns) */
    int32_t device;    /* HIP device ordinal */
    int32_t max_k;     /* default 3; 0 = univariate network only */
    int32_t hps;       /* default 5 (heuristic power size, src/tests.jl:5-6) */
    int32_t fdr;       /* default 1: Benjamini-Hochberg on level-0 p-values (src/tests.jl:521-529) */
    int32_t dense_rules; /* FW_MI / FW_MI_NZ only.  0 (default): contingency tables follow the SparseMatrixCSC methods
                          * (src/contingency.jl:80-480), what learn_network uses (make_sparse = true).  1: the dense
                          * Matrix methods (src/contingency.jl:7-56 + level_map! src/misc.jl:162-184): every row is
                          * visited and levels_z = number of distinct Z keys over all rows.  The cell counts
                          * are the same; only levels_z (power verdict) can differ, and only for FW_MI_NZ.
                          * fw_learn_network with FW_MI_NZ + dense_rules tests on the per-(target, candidate) row views of
                          * src/hiton.jl:41-50 (see fw_set_row_views). */
    int64_t n_obs_min; /* default -1 = automatic (src/learning.jl:51-64, fires for every test kind) */
    int64_t max_tests; /* default 10_000_000 per (T, candidate) pair (src/learning.jl:205) */
    double alpha;      /* default 0.01 */
    int32_t recursive_pcor; /* FW_FZ and FW_FZ_NZ (r04: for FW_FZ_NZ the correlations of a job's ROW VIEW, hiton.jl:85, in Float64,
                             * conditioned as StatsBase.partialcor does, with the view's own sample size).  1 (default): conditional tests are recursive partial correlations on the resident
                             * Pearson matrix (pcor_rec, src/statfuns.jl:23-75).  0: no correlation matrix is used for them --
                             * every test streams its k + 2 sample columns from HBM and computes the partial correlation from
                             * the data (pcor -> StatsBase.partialcor, src/statfuns.jl:19-21; the FzTestCond with an empty
                             * cor_mat of src/tests.jl:253, learn_network(recursive_pcor = false)).  Level 0 keeps the matrix. */
    int32_t no_cor_mat;     /* FW_FZ with recursive_pcor = 0 only.  0 (default, the reference's dense_cor = true): level 0 reads the
                             * resident p x p Pearson matrix (src/learning.jl:42-45).  1 (dense_cor = false, src/tests.jl:118-147 with an
                             * empty cor_mat): no matrix exists at any time -- fw_level0 multiplies the centred columns tile by tile
                             * on the matrix cores and screens every tile in the epilogue (the same Float32 correlations and
                             * thresholds as the matrix path, hence the same network as no_cor_mat = 0), conditional tests come
                             * from the data (recursive_pcor = 0).  p is then bounded by the data (2 x n x p floats), not by p^2.
                             * fw_compute_cor_mat / fw_set_cor_mat / fw_get_cor_mat / fw_use_cor_buffer fail with FW_ERR_STATE. */
} fw_params;

/* One TestResult (src/types.jl:140-145) */
typedef struct fw_test_result {
    double stat;
    double pval;
    int32_t df;
    int32_t suff_power; /* 0 / 1 */
} fw_test_result;

/* Return of test_subsets (src/tests.jl:281-346): (TestResult, Zs, num_tests, fraction) */
#define FW_SUBSETS_EMPTY 0    /* Z_total was empty: sentinel (NaN, NaN, -1, true), (-1,), -1, NaN (src/tests.jl:285) */
#define FW_SUBSETS_STOPPED 1  /* returned at the first non-significant test or at max_tests (:326-336) */
#define FW_SUBSETS_ALL_SIG 2  /* every subset significant: the max-p result (:338-345) */
typedef struct fw_subsets_result {
    double stat;
    double pval;
    int32_t df;
    int32_t suff_power;
    int32_t status;          /* FW_SUBSETS_* */
    int32_t n_zs;            /* length of zs */
    int32_t zs[FW_MAX_K];    /* conditioning set of the returned result (variable ids) */
    int32_t reserved0;
    int64_t num_tests;       /* tests executed in the reference's sequential order (-1 for EMPTY) */
    double frac;             /* num_tests / total number of subsets */
} fw_subsets_result;

/* Counters the metric needs (the reference has none) */
typedef struct fw_counters {
    int64_t level0_tests;        /* p(p-1)/2 pair tests issued */
    int64_t cond_tests_ref;      /* sum of num_tests over all test_subsets calls (reference-equivalent) */
    int64_t cond_tests_evaluated;/* tests actually evaluated on the device (includes speculation) */
    int64_t subsets_calls;       /* number of (T, candidate) jobs */
    int64_t kernel_launches;
    int64_t subsets_launches;    /* launches of the test_subsets segment kernel */
    double t_level0_s;           /* wall seconds inside fw_level0 */
    double t_level0_host_s;      /* of which: host-side BH + neighbour-list construction */
    double t_cond_s;             /* wall seconds inside the conditional stage of fw_learn_network */
    double t_dev_subsets_s;      /* HIP-event seconds of the test_subsets kernels (sum) */
    double t_host_advance_s;     /* host: HITON-PC state machines + job posting */
    double t_host_build_s;       /* host: segment construction + staging */
    double t_host_launch_s;      /* host: enqueueing copies + kernel */
    double t_host_wait_s;        /* host: waiting for the device (copies + kernel + sync) */
    double t_host_merge_s;       /* host: in-order merge of segment outputs */
    double alg_bytes_subsets;    /* algorithmic bytes of the evaluated conditional tests:
                                    fz: 4*C(k+2,2)+32 per test of order k; discrete: (k+2)*n*b/8+32, b = 1 (mi) / 2 (mi_nz) */
    /* ABI 5 -- recursive_pcor = 0 with job-local correlation matrices (the default form of that variant): its own algorithmic unit.
     * A (T, candidate | subsets of a accepted variables) job computes ONE (a+2) x (a+2) matrix from its columns and every test
     * conditions a sub-matrix of it, so what must cross HBM is the job's columns once, and the contraction is 2 n C(a+2, 2) flops;
     * alg_bytes_subsets (columns per TEST) stays the unit of the streamed form (FW_FZS_GRAM=0, explicit test batches). */
    int64_t gram_jobs;           /* job matrices computed */
    double gram_alg_bytes;       /* sum over them of (a + 2) * n * 4 */
    double gram_alg_flops;       /* sum over them of 2 * n * C(a + 2, 2) */
    /* ABI 6 -- level 0 of the discrete kinds on the matrix cores (mi_level0_mfma_kernel): the binary Gram product, priced against the
     * dense fp4 peak */
    double l0_mfma_flops;        /* 2 x multiply-adds issued: tiles x 256 x 256 plane rows x 64 W samples (padded words included) */
    double t_l0_mfma_s;          /* HIP-event seconds of the kernel's launches */
} fw_counters;

/* ---- lifecycle -------------------------------------------------------------------------------- */

/* Fills *params with the reference defaults for `kind`. */
void fw_params_default(fw_params *params, int32_t kind, int32_t n, int32_t p);

/* replaces: make_test_object (src/misc.jl:34-45) + the per-worker data hand-over (src/interleaved.jl:90-93).
 * On failure *out is NULL and fw_last_error(NULL) describes the problem. */
int fw_ctx_create(const fw_params *params, fw_ctx **out);
int fw_ctx_destroy(fw_ctx *ctx);
const char *fw_last_error(const fw_ctx *ctx); /* ctx may be NULL: last creation error of this thread */
int fw_abi_version(void);

/* ---- data ------------------------------------------------------------------------------------- */

/* FW_FZ: the normalised dense matrix (Matrix{Float32}, n x p column-major) the reference hands to
 * cor() in prepare_lgl (src/learning.jl:42-45).  FW_FZ_NZ: the clr_nz matrix with zeros = absences (the reference
 * holds it as SparseMatrixCSC{Float32}; fw_set_data_csc_f32 takes it in that form). */
int fw_set_data_dense_f32(fw_ctx *ctx, const float *data);

/* FW_FZ_NZ only (FW_ERR_ARG on any other kind): the clr_nz matrix as SparseMatrixCSC{Float32,Int64} with 0-based colptr / rowval.  The
 * triple is copied to the device and scattered there into the resident layout of fw_set_data_dense_f32 (values [p][n] and the plane
 * of values != 0): the host never holds n x p floats, and the two uploads of one matrix leave identical device bytes.  A stored
 * 0.0f means what a 0.0f cell means to the dense upload: an absence.  colptr must be monotone from 0 to nnz and the rows of a
 * column strictly ascending in 0 .. n-1 (checked on the device, one pass): otherwise FW_ERR_ARG, the message names the first bad
 * column, and the context holds no data until the next successful upload. */
int fw_set_data_csc_f32(fw_ctx *ctx, const int64_t *colptr, const int32_t *rowval, const float *nzval);

/* FW_FZ_NZ only (FW_ERR_ARG on any other kind): the same triple, kept sparse on the device -- the CSC-resident layout.  Resident are
 * the plane of values != 0 ([p][W] 64-bit words, W = ceil(n / 64)), base[p][W] (uint32: the position in `vals` of the column's first
 * entry at or after row 64 w) and vals (the values != 0.0f, column after column, rows ascending): 12 p W + 4 nnz' bytes instead of
 * 4 n p + 8 p W, nnz' = the number of values != 0; the n x p matrix is never allocated, and neither rowval nor colptr stays resident.
 * A stored 0.0f (and -0.0f) is an absence and is dropped while the layout is built.  Level 0, fw_test_batch, fw_test_subsets_batch
 * and fw_learn_network* run the same kernels with another load of each value: results are the bits of the dense-resident layout.
 * The triple is checked as fw_set_data_csc_f32 checks it (same messages); a refused triple leaves the context as it was.  An upload
 * of either layout replaces what the other held.  FW_ERR_LIMIT: nnz' >= 2^32, and recursive_pcor = 0 (the message names it; its
 * kernels stream whole dense columns). */
int fw_set_data_csc_f32_resident(fw_ctx *ctx, const int64_t *colptr, const int32_t *rowval, const float *nzval);

/* FW_FZ_NZ: bytes of device memory the context holds for the data, as asked of the allocator -- dense-resident: 4 n p (values) +
 * 8 p W (plane); CSC-resident: 4 max(nnz', 1) (vals) + 8 p W (plane) + 4 p W (base).  FW_ERR_STATE before the first upload. */
int fw_data_resident_bytes(const fw_ctx *ctx, int64_t *bytes);

/* FW_MI / FW_MI_NZ: SparseMatrixCSC{Int32,Int64} as produced by normalize_data (make_sparse = true).
 * colptr has p+1 entries; rowval is 0-based and sorted within each column; values are 1..61, stored
 * zeros are not allowed.  Values 1..2 everywhere (presence / absence, the two bins of binned_nz_clr): two bit planes per variable, the
 * fast kernels.  A value above 2 anywhere (meta variables with make_onehot = false, src/preprocessing.jl:42-117): the GENERIC form -- one
 * byte per value, tables of L x L x L^k cells as src/types.jl:98-117 sizes them, L = maximum + 1 <= 62; a test's table of L^max_k (L^2 + 1) words sits in LDS up to 3845
 * words and in device memory up to 64 M words (r05), else FW_ERR_LIMIT; same entry points and results, HITON-PC through the host job pool.
 * Also computes levels / max_vals (src/misc.jl:64-97). */
int fw_set_data_csc_i32(fw_ctx *ctx, const int64_t *colptr, const int32_t *rowval, const int32_t *nzval);

/* FW_MI / FW_MI_NZ, dense input (Matrix{Int32}, n x p column-major, values 0..61, see above); converted on the host to
 * the same packed device layout, i.e. evaluated with the SPARSE-path semantics (levels_z rules). */
int fw_set_data_dense_i32(fw_ctx *ctx, const int32_t *data);

/* Tables that already live in device memory (a torch tensor's data_ptr(), a ROCArray's pointer): column-major [p][n] on the
 * context's device.  The pointer is asked of the runtime (hipPointerGetAttributes) before anything reads it: NULL, a host pointer
 * and memory of another device give FW_ERR_ARG without a dereference.  The table is borrowed for the call only; the call
 * synchronises before it returns, so the caller may free or reuse the buffer at once.  Work of the caller's own streams that
 * produces the table must be complete before the call.
 * fw_set_data_dense_i32_dev (FW_MI / FW_MI_NZ): the resident layouts of fw_set_data_csc_i32 built on the device in two passes -- a
 * column scan (range check, the values seen, the totals), of which only p small records reach the host, which picks the form, fills
 * levels / max_vals and refuses as fw_set_data_dense_i32 refuses the same table (same code, same message: the lowest bad column and
 * the value at its first bad row); then the pack: one wavefront per plane word, the two ballots of 64 consecutive rows being the two
 * plane words (three-level form), or a cast to the byte matrix (generic form).  The host never holds n x p cells.
 * fw_set_data_dense_f32_dev (FW_FZ / FW_FZ_NZ): a device-to-device copy into the resident matrix and, for FW_FZ_NZ, the plane of
 * x != 0.0f by the same ballot scheme (-0.0f is an absence, a NaN is not, as in fw_set_data_dense_f32); FW_ERR_STATE in Float64 mode.
 * Either leaves the context in the state its host sibling leaves for the same table, to the bit. */
int fw_set_data_dense_i32_dev(fw_ctx *ctx, const int32_t *d_data);
int fw_set_data_dense_f32_dev(fw_ctx *ctx, const float *d_data);

/* Sparse tables that already live in device memory (the three arrays of a sparse CSC torch tensor, of a CuSparseMatrixCSC-like ROCm
 * array): d_colptr[p + 1] Int64, d_rowval[nnz] Int32, 0-based, and d_nzval[nnz], on the context's device, borrowed for the call only
 * (the streams' rule is that of the dense _dev forms).  nnz is passed: the size of the two arrays.  Every pointer is asked of the
 * runtime before anything reads it (NULL, a host pointer, memory of another device: FW_ERR_ARG without a dereference; d_rowval and
 * d_nzval may be NULL when nnz == 0).  Then the p + 1 column pointers are downloaded, and FW_ERR_ARG is returned unless they run
 * monotonically from 0 to nnz -- before any kernel reads d_rowval or d_nzval, so no kernel ever indexes outside the two arrays.  Nothing
 * else of the triple crosses to the host, and the triple is not copied in device memory: what the uploads stage there is small and
 * per column (the p column flags and the total in the FW_FZ_NZ forms, the p scan records in the discrete form).  The triple must be
 * canonical (rows strictly ascending within a column, no duplicates): it is checked, not repaired.
 * fw_set_data_csc_f32_dev / fw_set_data_csc_f32_resident_dev (FW_FZ_NZ): the kernels of fw_set_data_csc_f32 /
 * fw_set_data_csc_f32_resident on the borrowed triple -- the same resident bytes, state rules, refusals and limits (a stored 0.0f or
 * -0.0f is an absence; a refused triple leaves the context without data / as it was; recursive_pcor = 0 on the resident layout is
 * FW_ERR_LIMIT).
 * fw_set_data_csc_i32_dev (FW_MI / FW_MI_NZ): the resident layouts of fw_set_data_csc_i32 in the two passes of
 * fw_set_data_dense_i32_dev.  Scan, one wavefront per column: the column's range, then one pass over its rows and stored values; p small records reach the
 * host (value mask, counts, maximum, first defect), which picks the form, fills levels / max_vals (the distinct stored values, plus one
 * when the column has fewer than n entries) and refuses with the code fw_set_data_csc_i32 gives the same defect, naming the column:
 * rows unsorted or out of range FW_ERR_ARG, a stored zero or a value outside 1 .. 61 FW_ERR_LIMIT.  Pack, three-level form: every lane
 * owns one plane word, finds its entries in the column's sorted run by binary search and writes the two words whole (no atomics, no
 * clearing; pad columns and slack words come out zero).  Generic form: the byte matrix is cleared and scattered, one wavefront per
 * column.  A refused triple leaves the context as it was. */
int fw_set_data_csc_i32_dev(fw_ctx *ctx, const int64_t *d_colptr, const int32_t *d_rowval, const int32_t *d_nzval, int64_t nnz);
int fw_set_data_csc_f32_dev(fw_ctx *ctx, const int64_t *d_colptr, const int32_t *d_rowval, const float *d_nzval, int64_t nnz);
int fw_set_data_csc_f32_resident_dev(fw_ctx *ctx, const int64_t *d_colptr, const int32_t *d_rowval, const float *d_nzval, int64_t nnz);

int fw_get_levels(const fw_ctx *ctx, int32_t *levels, int32_t *max_vals); /* p entries each */

/* FW_FZ: supply a precomputed Pearson matrix (p x p, Float32) instead of computing it on the device --
 * mirrors `cor_mat` being an argument of pw_univar_neighbors / si_HITON_PC (src/tests.jl:441, src/hiton.jl:284). */
int fw_set_cor_mat(fw_ctx *ctx, const float *cor_mat);
/* replaces: cor(data_dense) -> Matrix{Float32} (src/learning.jl:44).  MFMA kernel; result stays resident. */
int fw_compute_cor_mat(fw_ctx *ctx);
int fw_get_cor_mat(const fw_ctx *ctx, float *cor_mat_out); /* p*p floats */

/* ---- Float64 mode of FW_FZ: learn_network(prec = 64), cont_type = Float64 (src/learning.jl:42-45; pcor_rec then runs and rounds in
 * Float64, src/statfuns.jl:23-75).  The first call of fw_set_data_dense_f64 or fw_set_cor_mat_f64 puts the context in Float64 mode for
 * good: the p x p matrix is resident as Float64 (8 p^2 bytes; FW_ERR_NOMEM beyond what the device has) and fw_compute_cor_mat,
 * fw_level0, fw_level0_get, fw_test_batch, fw_test_subsets_batch, fw_learn_network, fw_network_get*, fw_set_track_rejections and the
 * counters work on it with unchanged signatures (HITON-PC through the host job pool).
 * Precisions never mix and nothing is cast: the _f64 setters on a context that holds Float32 input, fw_set_data_dense_f32 /
 * fw_set_cor_mat / fw_get_cor_mat on a Float64 context and fw_get_cor_mat_f64 on a Float32 context fail with FW_ERR_STATE; the _f64
 * setters on a context that is not FW_FZ with FW_ERR_ARG.
 * Not served in Float64 mode (FW_ERR_LIMIT, the message names the option): recursive_pcor = 0, no_cor_mat = 1, max_k above 5,
 * fw_use_cor_buffer, fw_compute_cor_mat_rows, fw_level0_sharded*, fw_learn_network_dev and the fw_*_comm entry points. */
int fw_set_data_dense_f64(fw_ctx *ctx, const double *data);        /* n x p column-major, Matrix{Float64} */
int fw_set_cor_mat_f64(fw_ctx *ctx, const double *cor_mat);        /* p x p, entries in [-1, 1] or NaN */
int fw_get_cor_mat_f64(const fw_ctx *ctx, double *cor_mat_out);    /* p*p doubles */

/* Exchange callback for target-sharded runs: called once per feed-forward round with this rank's newly found
 * directed neighbour entries (target, neighbour, weight-stat, p); must return the concatenation over all ranks
 * (rank order) through *out_* buffers allocated by the callee and valid until the next call.  NULL for
 * world_size = 1.  (RCCL all_gather in bench.py; gloo in the CPU tests.) */
typedef int (*fw_allgather_fn)(void *user, int64_t n_local, const int32_t *tgt, const int32_t *nbr, const double *stat,
                               const double *pval, int64_t *n_total, const int32_t **tgt_all, const int32_t **nbr_all,
                               const double **stat_all, const double **pval_all);

/* ---- level 0 ---------------------------------------------------------------------------------- */

/* replaces: pw_univar_neighbors (src/tests.jl:436-532) incl. the power/NaN rules and
 * benjamini_hochberg! (src/statfuns.jl:326-350).  Runs all p(p-1)/2 univariate tests on the device and
 * keeps the neighbour lists in the context.  *nnz_out = total number of (directed) neighbour entries. */
int fw_level0(fw_ctx *ctx, int64_t *nnz_out);
/* Same result, for target-sharded runs (one process per GPU): this rank screens only its share of the pair tiles (discrete
 * kinds; the Fisher-z kinds stay replicated) and the significant pairs are exchanged through the same callback type as the
 * per-round neighbour sets (fw_allgather_fn above: entries (i, j, stat, p)); Benjamini-Hochberg and the neighbour lists are
 * then built on every rank from the merged list.  The role of the reference's master process, which runs
 * pw_univar_neighbors once and ships the result to the workers (src/learning.jl:130-150, src/interleaved.jl:90-93). */
int fw_level0_sharded(fw_ctx *ctx, int32_t rank, int32_t world_size, fw_allgather_fn allgather, void *user, int64_t *nnz_out);
/* Device-resident exchange for target-sharded runs: the caller owns the communication buffers in DEVICE memory (torch tensors in
 * bench.py, all-gathered by RCCL over xGMI), the library packs into / unpacks from them with its own kernels -- no host copy of the
 * payload.  prepare(): every rank reports its record count and one auxiliary integer; the callee all-gathers both (counts[],
 * aux[], world_size entries each), makes room for cap = max(count) records of rec_bytes bytes in a send buffer and for world_size
 * blocks of cap records in a receive buffer, and returns their device addresses.  exchange(): all-gather the send buffers
 * (cap * rec_bytes bytes per rank) into the receive buffer in rank order; returns when the data is in place. */
typedef struct fw_dev_exchange {
    void *user;
    int (*prepare)(void *user, int64_t n_local, int64_t aux_local, int32_t rec_bytes, void **d_send, void **d_recv, int64_t *counts,
                   int64_t *aux, int64_t *cap_records);
    int (*exchange)(void *user);
} fw_dev_exchange;
/* fw_level0_sharded with the payload kept on the device: this rank screens its share of the pair tiles (discrete kinds), the
 * significant pairs are packed into the caller's send buffer, gathered, and Benjamini-Hochberg + the neighbour lists are built
 * from the gathered buffer on every rank.  (The Fisher-z kinds stay replicated: see fw_compute_cor_mat_rows for their share.) */
int fw_level0_sharded_dev(fw_ctx *ctx, int32_t rank, int32_t world_size, const fw_dev_exchange *exchange, int64_t *nnz_out);

/* FW_FZ, row-block sharding of cor(data_dense) (src/learning.jl:44) over the ranks: fw_use_cor_buffer makes the context keep its
 * p x p matrix in caller-owned device memory (capacity in floats >= world_size * rows_per_rank * p, see below);
 * fw_compute_cor_mat_rows computes the rows [*row0, *row0 + *rows_per_rank) of this rank (whole rows, no mirrored writes:
 * rows_per_rank = 128 * ceil(ceil(p / 128) / world_size), the same on every rank) and leaves the rest untouched; the caller then
 * all-gathers the row blocks in place (contiguous: rows_per_rank * p floats per rank) and calls fw_cor_mat_ready. */
int fw_use_cor_buffer(fw_ctx *ctx, void *d_cor, int64_t capacity_floats);
int fw_compute_cor_mat_rows(fw_ctx *ctx, int32_t rank, int32_t world_size, int64_t *row0, int64_t *rows_per_rank);
int fw_cor_mat_ready(fw_ctx *ctx);

/* Neighbour lists as CSR: off[p+1]; idx/stat/adj_p have nnz entries, partners ascending per variable;
 * adj_p is the BH-adjusted p-value when fdr = 1 (src/tests.jl:372-388). */
int fw_level0_get(const fw_ctx *ctx, int64_t *off, int32_t *idx, double *stat, double *adj_p);

/* ---- the per-pair test batch ------------------------------------------------------------------- */

/* replaces: test(X, Y, Zs, data, test_obj, ...) (src/tests.jl:28,108 for empty Zs; :184,:250 otherwise).
 * Test i is (X[i], Y[i] | zflat[zoff[i] .. zoff[i+1])), Z order preserved.  zoff has m+1 entries. */
int fw_test_batch(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff,
                  const int32_t *zflat, fw_test_result *out);

/* replaces: test_subsets(T, candidate, accepted, data, test_obj, max_k, alpha; hps, n_obs_min, max_tests)
 * (src/tests.jl:281-346) for m independent (T, candidate, accepted) jobs -- the call edge hiton.jl:100.
 * Job i conditions on accflat[accoff[i] .. accoff[i+1]) (acceptance order preserved, duplicates allowed).
 * Enumeration order, early exit and the `>=` max-p rule are the reference's; num_tests is the count the
 * sequential reference would have executed. */
int fw_test_subsets_batch(fw_ctx *ctx, int64_t m, const int32_t *T, const int32_t *cand, const int64_t *accoff,
                          const int32_t *accflat, fw_subsets_result *out);

/* FW_MI_NZ with dense_rules = 1 only.  hiton.jl hands test_subsets not the data but a row VIEW of it: the rows where T is
 * non-zero if T has more than two levels, and likewise for the candidate (prepare_nzdata, src/hiton.jl:41-50,85,193 ->
 * needs_nz_view, src/misc.jl:103-107).  on = 1: fw_test_subsets_batch evaluates job (T, candidate, .) on that view (what a
 * GpuTest shim called from hiton.jl:100 needs); on = 0 (default): on every row of the uploaded matrix (what a direct
 * test_subsets(T, candidate, Z, data, ...) call on the full matrix computes).  fw_learn_network always uses the views. */
int fw_set_row_views(fw_ctx *ctx, int32_t on);

/* ---- host driver: the caller side, for hosts without Julia ----------------- */

typedef struct fw_learn_opts {
    int32_t feed_forward;  /* default 1 (src/learning.jl:469) */
    int32_t round_size;    /* targets per feed-forward round; 1 = the reference's deterministic single_il schedule;
                              0 = one round (no whitelist can form: identical to feed_forward = 0 / parallel="single") */
    int32_t rank;          /* this process' rank in a target-sharded run (0 for single GPU) */
    int32_t world_size;    /* number of ranks; the targets of a round are dealt by estimated work (heaviest first to the least loaded rank) */
    int32_t max_targets;   /* > 0: stop after this many targets of the schedule (sampling; 0 = all) */
    int32_t elim_mode;     /* HITON-PC elimination phase (src/hiton.jl:53-78,388-390; was reserved0, zero keeps its meaning):
                              0 = fast_elim = true (default); 1 = fast_elim = false: a rejected member re-enters the conditioning
                              pool but not PC; 2 = fast_elim = false, no_red_tests = false: as 1, and PC keeps the elimination-phase
                              statistics (update_PC_dict! skipped).  Anything else: FW_ERR_ARG */
} fw_learn_opts;

/* replaces: LGL minus normalisation (src/learning.jl:203-279): level 0 (if not yet run), target ordering,
 * HITON-PC per target (src/hiton.jl:283-400) in level-synchronous batches over fw_test_subsets_batch,
 * feed-forward rounds (src/interleaved.jl:112-183), make_weights + make_symmetric_graph (src/misc.jl:137-272).
 * *n_edges_out = number of undirected edges; fetch them with fw_network_get. */
int fw_learn_network(fw_ctx *ctx, const fw_learn_opts *opts, fw_allgather_fn allgather, void *user,
                     int64_t *n_edges_out);
/* The same with the per-round exchange through a fw_dev_exchange (see fw_level0_sharded_dev): the round's directed entries are packed
 * into 24-byte records (int32 target, int32 neighbour, Float64 statistic, Float64 p) by the library, copied into the caller's device
 * send buffer, all-gathered by the caller's collective and unpacked from the gathered buffer -- the host language only runs the
 * collective (r02's callback packed and unpacked in numpy: ~0.9 ms per round of a cfg3 pass). */
int fw_learn_network_dev(fw_ctx *ctx, const fw_learn_opts *opts, const fw_dev_exchange *exchange, int64_t *n_edges_out);
/* replaces: si_HITON_PC(T, data; ...) (src/hiton.jl:402-409) for a list of targets: level 0 over all pairs (if not yet run), then
 * HITON-PC for the n_targets variables targets[0 .. n_targets) only, each on its own (no feed-forward: the reference's convenience
 * function passes an empty whitelist), then make_weights + make_symmetric_graph over those rows alone.  A listed target's directed row
 * is its row of fw_learn_network with feed_forward = 0, to the bit; the rows of the other variables are empty, so an edge to an
 * unlisted variable has one direction only.  The rejection log holds the listed targets' records.  max_k = 0: the targets' level-0
 * rows.  The targets run in the order of the schedule (ascending level-0 degree, stable), whatever the order of the list; nothing
 * is launched or counted for an unlisted variable.  Afterwards fw_network_get, fw_network_get_directed and the fw_rejections_*
 * getters work as after fw_learn_network; a later fw_learn_network or fw_learn_neighbors replaces the result and reuses level 0 and
 * the Pearson matrix.
 * opts: NULL means feed_forward = 0, round_size = 0, elim_mode = 0.  round_size only batches the work and does not change a bit.
 * FW_ERR_ARG, the message naming the field or the entry: a NULL context, NULL targets, n_targets < 1, an id outside 0 .. p-1, a
 * duplicate id, feed_forward != 0, world_size > 1, rank != 0, max_targets != 0, elim_mode outside 0 .. 2.  One rank only: there is no
 * sharded or communicator form. */
int fw_learn_neighbors(fw_ctx *ctx, const fw_learn_opts *opts, const int32_t *targets, int32_t n_targets, int64_t *n_edges_out);
/* ---- library-side collectives (ABI 5): the same exchanges on a communicator the LIBRARY owns ------------------------------------
 * replaces: the master <-> worker message loop of src/interleaved.jl:112-183 for one process per GPU.  RCCL (librccl.so.1, reached
 * through dlopen: single-GPU users never load it) on the context's stream; the host language only carries the 128-byte rendezvous
 * id from rank 0 to the others (torch.distributed / MPI / Distributed.jl) and never sees a payload.
 *   fw_comm_unique_id   rank 0: ncclGetUniqueId
 *   fw_comm_init        every rank, after fw_ctx_create on ITS device: ncclCommInitRank (one rank per device)
 *   fw_level0_comm      = fw_level0_sharded_dev with the library's all-gather (discrete kinds; Fisher-z kinds: plain fw_level0)
 *   fw_cor_mat_allgather_comm  the in-place all-gather of the row blocks of fw_compute_cor_mat_rows (then fw_cor_mat_ready)
 *   fw_learn_network_comm      = fw_learn_network_dev with the library's all-gather per feed-forward round; opts->rank /
 *                              world_size are taken from the communicator
 *   fw_comm_stats       exchanges so far: calls, collectives, directed entries, gathered bytes, seconds inside them */
#define FW_COMM_ID_BYTES 128
int fw_comm_unique_id(uint8_t *id128);
int fw_comm_init(fw_ctx *ctx, const uint8_t *id128, int32_t rank, int32_t world_size);
int fw_comm_destroy(fw_ctx *ctx);
int fw_comm_stats(const fw_ctx *ctx, int64_t *calls, int64_t *collectives, int64_t *entries, int64_t *bytes, double *seconds);
int fw_level0_comm(fw_ctx *ctx, int64_t *nnz_out);
int fw_cor_mat_allgather_comm(fw_ctx *ctx, int64_t rows_per_rank);
int fw_learn_network_comm(fw_ctx *ctx, const fw_learn_opts *opts, int64_t *n_edges_out);

int fw_network_get(const fw_ctx *ctx, int32_t *src, int32_t *dst, double *weight); /* src < dst */
/* directed per-target results (state_results of every HitonState): CSR over targets */
int fw_network_get_directed(const fw_ctx *ctx, int64_t *off, int32_t *idx, double *weight, double *pval);

/* ---- rejection log: learn_network(track_rejections = true), src/learning.jl:446,469 --------------------------------------------
 * One entry of rejections(net_result)[target][candidate] (RejDict, src/types.jl:152): update_sig_result! (src/hiton.jl:53-78) stores
 * it when a candidate is tested against a non-empty accepted list and the returned test is not significant -- the FIRST such test in
 * the order of test_subsets (src/tests.jl:281-346).  zs is that test's conditioning set in the order `combinations` yields it,
 * num_tests the count up to and including it, frac = num_tests / (number of subsets of sizes 1..max_k of the n_acc accepted variables,
 * not capped by max_tests).  A job that ends without a test (src/tests.jl:293-296) gives n_zs = 0, num_tests = 0, frac = 0.
 * Whitelisted candidates, the empty-pool acceptance and univariate non-significance leave no entry; a candidate is rejected at most
 * once per target.  88 bytes, no padding. */
typedef struct fw_rejection {
    int32_t target, candidate;
    int32_t n_zs;
    int32_t zs[FW_MAX_K];
    int32_t df, suff_power;
    int32_t phase;  /* 0 interleaving, 1 elimination (the reference does not keep it) */
    int32_t n_acc;  /* length of the accepted list the candidate was tested against (the reference does not keep it) */
    int64_t num_tests;
    double frac;
    double stat, pval;
} fw_rejection;
/* on = 1: the following fw_learn_network* calls keep the log (default 0; a switch of the context like fw_set_row_views, so that
 * fw_learn_opts keeps its layout).  The log is a diagnostic mode: the network is the same bytes either way.  In a target-sharded run
 * every rank holds the entries of its own targets until fw_rejections_allgather_dev / _comm (below) gives every rank all of them. */
int fw_set_track_rejections(fw_ctx *ctx, int32_t on);
/* entries of the last fw_learn_network* (0 if it ran with tracking off); FW_ERR_STATE before the first tracked run */
int fw_rejections_count(const fw_ctx *ctx, int64_t *n);
/* out[0 .. n): ascending (target, candidate) */
int fw_rejections_get(const fw_ctx *ctx, fw_rejection *out);
/* Target-sharded runs: the whole log on every rank, as the reference's master collects every worker's rej_dict (src/learning.jl:196-199).
 * COLLECTIVE: every rank of the run calls it once, after a tracked fw_learn_network_dev / _comm (or fw_learn_network with
 * world_size > 1); a rank with nothing logged (max_k = 0, no record of its own) takes part with 0 records.  Afterwards
 * fw_rejections_count / fw_rejections_get return the entries of ALL targets on every rank -- ascending (target, candidate), frac filled:
 * the bytes of a one-rank log wherever the run's tests are.  The payload stays in device memory: the filled slots are packed into the
 * exchange's send buffer as 96-byte records (the 88 bytes + the slot index), gathered, and scattered into this rank's slots by
 * csrc/fw_xchg.hip.  A second call is a no-op (FW_OK, no collective); without the call nothing changes: every rank keeps the entries of
 * its own targets.  FW_ERR_STATE before the first tracked run (and when fw_level0 ran again since it); FW_ERR_ARG for a NULL exchange
 * and for _comm without a communicator (fw_comm_init); FW_ERR_DEVICE, with a message, when two ranks deliver a record for one slot --
 * targets are dealt to one rank each, no winner is picked. */
int fw_rejections_allgather_dev(fw_ctx *ctx, const fw_dev_exchange *exchange);
int fw_rejections_allgather_comm(fw_ctx *ctx); /* the same on the library's own communicator (fw_comm_init) */
/* the last gather of this context: records this rank packed that the host job pool / the device paths had written, and records of
 * other ranks placed here; FW_ERR_STATE when the log is not a gathered one */
int fw_rejections_allgather_stats(const fw_ctx *ctx, int64_t *packed_host, int64_t *packed_dev, int64_t *received);

/* ---- normalisation front-end on the device -------------------------------------- */

/* replaces: normalize_data / preprocess_data (src/preprocessing.jl:412-563) for a count table without meta variables:
 * filter_by_variance (:367-409), then by kind  FW_FZ: clr_adapt (:133-214)   FW_FZ_NZ: clr_nz (:192-207)   FW_MI: binary (:475-490)
 * FW_MI_NZ: binned_nz_clr (clr_nz, then per column the tied ranks of the non-zero entries in two bins, :217-291,492-521; the
 * column sort runs in LDS up to 16 384 samples and through device memory beyond).  counts: n x p column-major Int32.  Outputs (host buffers sized for n x p): out_f32 (FW_FZ / FW_FZ_NZ) or
 * out_i32 (FW_MI / FW_MI_NZ), column-major *n_out x *p_out; row_mask[n] / col_mask[p] = kept samples / variables.  No context
 * needed: create one with the resulting shape afterwards.  Meta variables (a handful of columns) are prepared by the caller
 * (one-hot, discretisation: preprocess.py) and appended.
 * kind may also be one of the two total-sum-scaling transforms (norm_mode of normalize_data, :660-684), under the same filters:
 * FW_NORM_TSS ("rows", :348-361): out_f32 = (float)x / s_i, s_i the Float32 sum of sample i over the kept columns, added in ascending
 * column order from +0.0f, one IEEE Float32 division per cell -- the arithmetic stays in Float32 as the reference's does.
 * FW_NORM_TSS_BINNED ("binned_nz_rows", :492-521): out_i32 = FW_MI_NZ's ranks, bins and column rule with that quotient as the key.
 * The CSC siblings return both sparse (FW_NORM_TSS: Float32 values, a quotient that underflows to 0 is a stored 0.0f).  A kept
 * sample whose Float32 sum is 0 or infinite (real values outside the Float32 range) gives FW_ERR_ARG. */
int fw_normalize_counts(int32_t device, int32_t kind, int32_t n, int32_t p, const int32_t *counts, float *out_f32, int32_t *out_i32,
                        uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out);

/* The same front-end on a sparse count table (SparseMatrixCSC{Int32,Int64}, 0-based colptr[p+1] / rowval, counts 1 .. 2^31-1), as the
 * reference keeps heterogeneous data (make_sparse, src/learning.jl:470): O(nnz) work and memory on host and device, results bit-identical
 * to fw_normalize_counts on the dense form of the same table.  Checked on the device in one pass: a non-monotone colptr, a row
 * outside 0 .. n-1, unsorted or duplicate rows, a stored zero or a negative count give FW_ERR_ARG and the message names the first
 * bad column.  At most 2^31-1 stored entries (FW_ERR_LIMIT).
 * Outputs (host buffers): FW_MI / FW_MI_NZ: CSC Int32 out_colptr / out_rowval / out_i32 over the kept samples (renumbered) and
 * kept variables -- what fw_set_data_csc_i32 takes; FW_FZ_NZ: CSC Float32 with out_f32 as values -- what fw_set_data_csc_f32
 * takes; a kept entry whose clr_nz value is exactly 0 is a stored 0.0f; FW_FZ (clr_adapt, no cell is zero): dense *n_out x *p_out
 * column-major in out_f32, out_colptr / out_rowval unused.  out_colptr holds p+1 entries, out_rowval and the value buffer the
 * input's nnz (FW_FZ: n x p floats); the buffer of the other value type may be NULL.  *nnz_out = entries written. */
int fw_normalize_counts_csc(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval,
                            const int32_t *nzval, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32,
                            uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out);

/* The same two front-ends on a real-valued table (relative abundances, percentages, coverage-normalised counts, counts beyond
 * 2^31-1): the reference normalises any Real matrix, and adaptive_pseudocount! (:157-190) takes a tenth of the smallest abundance
 * as its floor when that lies below 1.  The same kernels instantiated for Float64 values (csrc/fw_norm.hip): contracts, outputs
 * and limits are those of the _counts siblings, and a table of integers gives the bits its Int32 form gives.  values / nzval:
 * Float64, each >= 0 and finite (-0.0 is a zero); a negative value, a NaN or an Inf gives FW_ERR_ARG naming the first offending
 * column (dense) or the column (CSC), as does a stored zero in the CSC form.  Integers beyond 2^53 are no longer exact.  The
 * variance filter stays min != max (a CSC column's implicit zeros counted): exact, where a floating-point variance of a constant
 * column can be a rounding residue.  Device memory: 8 bytes per dense cell (the count form takes 4); the CSC form holds 8 B per
 * stored value and sorts a 32-bit entry index with a 32-bit column per entry beside it, where the count form sorts one packed
 * 64-bit (column, count) word. */
int fw_normalize_abund(int32_t device, int32_t kind, int32_t n, int32_t p, const double *values, float *out_f32, int32_t *out_i32,
                       uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out);
int fw_normalize_abund_csc(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval,
                           const double *nzval, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32,
                           uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out);

/* The options of the two binned kinds (FW_MI_NZ, FW_NORM_TSS_BINNED): the reference's preprocess_kwargs n_bins, rank_method and
 * disc_method (discretize, :217-291; preprocess_data, :412-416,492-521).  b = n_bins - 1 is the number of non-zero bins; in every
 * kept column the keys of the non-zero entries (the clr_nz value, or the Float32 TSS quotient widened) are discretised in Float64:
 *   FW_DISC_MEDIAN  r = the tied (average) rank (FW_RANK_TIED) or the dense rank (FW_RANK_DENSE: the distinct keys numbered 1 .. d
 *                   in ascending order); level = floor((r / max r) / (1.0 / b + 1e-5)) + 1, in 1 .. b
 *   FW_DISC_MEAN    (n_bins = 3 only) level = key <= mean ? 1 : 2, the mean being the pairwise sum of the column's keys sorted
 *                   ascending and padded with +0.0 to the next power of two (a[2i] + a[2i+1], level by level), divided by their
 *                   number: one number on every path, within rounding of the reference's mean(); rank_method is not looked at
 * Zeros stay 0, and a column is kept iff its non-zero entries show exactly b distinct levels (:511-515).  Output: Int32 levels
 * 0 .. b.  The defaults {3, FW_RANK_TIED, FW_DISC_MEDIAN} are what the four entry points above compute, to the bit.
 * FW_ERR_ARG, the message naming the field, before any device call: n_bins outside 3 .. 62 (2 is FW_MI; the engine takes
 * variables of at most 62 levels), an unknown rank_method or disc_method, FW_DISC_MEAN with n_bins > 3, and any field away from its
 * default with a kind that does not bin. */
#define FW_RANK_TIED 0
#define FW_RANK_DENSE 1
#define FW_DISC_MEDIAN 0
#define FW_DISC_MEAN 1
typedef struct fw_norm_opts {
    int32_t n_bins, rank_method, disc_method;
} fw_norm_opts;

/* The four front-ends above with the options as a last argument (NULL: the defaults); the entry points above forward here with NULL. */
int fw_normalize_counts_opts(int32_t device, int32_t kind, int32_t n, int32_t p, const int32_t *counts, float *out_f32, int32_t *out_i32,
                             uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, const fw_norm_opts *opts);
int fw_normalize_counts_csc_opts(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval,
                                 const int32_t *nzval, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32,
                                 uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
                                 const fw_norm_opts *opts);
int fw_normalize_abund_opts(int32_t device, int32_t kind, int32_t n, int32_t p, const double *values, float *out_f32, int32_t *out_i32,
                            uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, const fw_norm_opts *opts);
int fw_normalize_abund_csc_opts(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval,
                                const double *nzval, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32,
                                uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
                                const fw_norm_opts *opts);

/* The dense front-ends on a table that already lives in device memory: d_counts / d_values is column-major [p][n] on `device` and is
 * borrowed, not uploaded; the output goes into the caller's device buffer of n p elements (d_out_f32 or d_out_i32 by kind, as above:
 * kept samples x kept columns, column-major, at its start) instead of being downloaded.  Both pointers are asked of the runtime
 * before anything reads them (FW_ERR_ARG for NULL, a host pointer, memory of another device).  The masks, the counts and opts stay on
 * the host; opts == NULL means the defaults.  The same kernels run in the same order as in fw_normalize_counts_opts /
 * fw_normalize_abund_opts, so the same bits come out; the small per-row and per-column statistics go through the host as they do
 * there.  Device memory besides the two buffers: the binned kinds' temporary of n p Int32.  The call synchronises before it returns. */
int fw_normalize_counts_dev(int32_t device, int32_t kind, int32_t n, int32_t p, const int32_t *d_counts, float *d_out_f32,
                            int32_t *d_out_i32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out,
                            const fw_norm_opts *opts);
int fw_normalize_abund_dev(int32_t device, int32_t kind, int32_t n, int32_t p, const double *d_values, float *d_out_f32,
                           int32_t *d_out_i32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out,
                           const fw_norm_opts *opts);

/* The CSC front-ends on a triple that already lives in device memory: the arguments of the *_csc_opts entry points, except that
 * d_colptr (Int64, p + 1), d_rowval (Int32, nnz) and d_nzval (Int32 | Float64, nnz) are device pointers on `device`, borrowed and not
 * uploaded; nnz is passed; and the outputs d_out_colptr (p + 1 entries), d_out_rowval (nnz), d_out_i32 | d_out_f32 (nnz; FW_FZ: n p
 * floats, d_out_colptr / d_out_rowval unused) are device buffers of the caller that the output kernels write in place, nothing is
 * downloaded.  row_mask, col_mask, n_out, p_out, nnz_out and opts (NULL: the defaults) stay on the host.  Every pointer is asked of
 * the runtime before anything reads it (FW_ERR_ARG for NULL, a host pointer, memory of another device); then the column pointers are
 * downloaded and FW_ERR_ARG is returned unless they run monotonically from 0 to nnz, before any kernel reads d_rowval or d_nzval.  The
 * same kernels run in the same order as in the host forms, so the same bits come out and the same defects are refused with the same
 * words; the per-column and per-row records go through the host as they do there.  The outputs must not overlap the inputs.  The
 * call synchronises before it returns. */
int fw_normalize_counts_csc_dev(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *d_colptr, const int32_t *d_rowval,
                                const int32_t *d_nzval, int64_t nnz, int64_t *d_out_colptr, int32_t *d_out_rowval, int32_t *d_out_i32,
                                float *d_out_f32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
                                const fw_norm_opts *opts);
int fw_normalize_abund_csc_dev(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *d_colptr, const int32_t *d_rowval,
                               const double *d_nzval, int64_t nnz, int64_t *d_out_colptr, int32_t *d_out_rowval, int32_t *d_out_i32,
                               float *d_out_f32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
                               const fw_norm_opts *opts);

/* Device self-test of hand-written arithmetic sequences that replace a compiler-generated IEEE sequence and must return the
 * same bits.  which = FW_SELFTEST_DIV: the unscaled Float64 division of the NaN-free partial-correlation path (statfuns.jl:44-62
 * `/`) against the compiler's division on `cases` hashed operand pairs of that path's ranges; *mismatches = pairs that differ. */
#define FW_SELFTEST_DIV 1
int fw_selftest(fw_ctx *ctx, int which, uint64_t cases, uint64_t seed, uint64_t *mismatches);

int fw_get_counters(const fw_ctx *ctx, fw_counters *out);
int fw_reset_counters(fw_ctx *ctx);
/* effective n_obs_min after the automatic rule */
int64_t fw_effective_n_obs_min(const fw_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* FLASHWEAVE_AMD_H */
