// Internal declarations shared by the translation units of libflashweave_amd.so.
// Nothing here is part of the ABI (include/flashweave_amd.h is).
#pragma once
// The library is written for gfx950 (MI355X, CDNA4) ONLY: mi_level0_mfma_kernel issues v_mfma_scale_f32_32x32x64_f8f6f4 and the kernels
// size their static LDS for 160 KB per CU.  There is no dual path; another --offload-arch fails here instead of deep inside a kernel.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libflashweave_amd targets gfx950 only (make ARCH=gfx950)"
#endif
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/flashweave_amd.h"
#include "fw_graph.h"  // host-only: FwDirected, FwNetwork, FwHostWorkers, fwi_now_s
#include "fw_pool_host.h"  // host-only: FwJob, FwJobOut, FwSeg, FwSegOut, FW_RANK_NONE, the job pool's rules
#include "fw_stage_host.h"  // host-only: the level-0 capacity policy (fw_l0_first_cap, fw_l0_attempts)

struct FwDevBuf {
    void *ptr = nullptr;
    size_t cap = 0;
};

struct FwPinned {
    void *ptr = nullptr;
    size_t cap = 0;
};

// A device array that owns its memory (move-only, hipFree in the destructor): the scratch of a host driver that returns on error.
// The copies are the synchronous hipMemcpy on the null stream; the caller maps the hipError_t to its code (FW_HIP, FW_HIP_MEM).
// release() hands the pointer on, e.g. into the context.
template <typename T> class FwDevArray {
    T *p_ = nullptr;

public:
    FwDevArray() = default;
    FwDevArray(FwDevArray &&o) noexcept : p_(o.release()) {}
    FwDevArray &operator=(FwDevArray &&o) noexcept
    {
        if (this != &o) {
            if (p_) (void)hipFree(p_);
            p_ = o.release();
        }
        return *this;
    }
    FwDevArray(const FwDevArray &) = delete;
    FwDevArray &operator=(const FwDevArray &) = delete;
    ~FwDevArray()
    {
        if (p_) (void)hipFree(p_);
    }
    hipError_t alloc(size_t count)
    {
        *this = FwDevArray();
        return hipMalloc((void **)&p_, sizeof(T) * count);
    }
    hipError_t upload(const T *src, size_t count)
    {
        const hipError_t e = alloc(count);
        return e != hipSuccess ? e : hipMemcpy(p_, src, sizeof(T) * count, hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
    hipError_t download(T *dst, size_t count) const { return hipMemcpy(dst, p_, sizeof(T) * count, hipMemcpyDeviceToHost); }
    hipError_t download(std::vector<T> &v) const { return download(v.data(), v.size()); }  // (v.size() elements)
    T *get() const { return p_; }
    T *release()
    {
        T *p = p_;
        p_ = nullptr;
        return p;
    }
};

// A table the *_dev entry points borrow: device memory of `device`, asked of the runtime before anything reads it.  NULL, a host
// pointer (pinned or not), managed memory and memory of another device are not.
inline bool fw_is_dev_ptr(const void *q, int device)
{
    if (!q) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, q) != hipSuccess) {
        (void)hipGetLastError();  // (an unregistered host pointer: the error is the answer, not a state to keep)
        return false;
    }
    return a.type == hipMemoryTypeDevice && a.device == device;
}

// Conditioning sets of 6 and 7 variables (ABI 6: FW_MAX_K = 7; tests.jl:311-343 has no cap) take general-form kernels through the host job
// pool; every table kernel, the device rounds and the persistent discrete kernel size their arrays for FW_MAX_K_FAST.
#define FW_MAX_K_FAST 5

#define FW_TAB_A 512  // fz / fz_nz: largest |accepted| served by the LDS-table kernel (csrc/fw_fz.hip, FZ_TAB_CAP)
#ifndef FW_HK_A
#define FW_HK_A 88    // fz, max_k 4-5: largest |accepted| served by the level-2 table kernel (one (z1, z2) table <= FZ_HK_CAP)
#endif

// Per-job record of the HE-S (fz_nz) path: the correlation sub-matrix of a job is computed over the rows where both
// T and the candidate are non-zero (statfuns.jl:138-155 cor_subset!), lives in a device arena and is indexed locally
// (0 = T, 1 = candidate, 2 + i = accepted[i]).
struct FwNzJob {
    int32_t X, Y;
    long long acc_off;  // into the flat accepted array of the launch
    int32_t acc_len;
    int32_t m;          // acc_len + 2
    long long cor_off;  // offset (floats) of the m x m matrix in the arena
    int32_t nR;         // rows with X != 0 and Y != 0            (device-computed)
    int32_t pad;
    double zscale;      // sqrt(nR - 3) / 2, 0 if nR <= 3          (device-computed)
    double rxy;         // unrounded Float64 pair correlation of (X, Y) over R, statfuns.jl:114 (device-computed)
    double thr[4];      // |r| significance thresholds for this nR (device-computed)
};

// per-pool staging: own stream + events so that two pools can be in flight (host merges one while the GPU runs the other)
// significant level-0 pairs as the kernels leave them in device memory (i < j; statistic in Float64 or Float32)
struct FwL0Dev {
    const int32_t *i = nullptr, *j = nullptr;
    const double *stat64 = nullptr;
    const float *stat32 = nullptr;
    const double *pval = nullptr;
    size_t k = 0;
};

struct FwPoolBuf {
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the segment kernel(s) of a launch
    hipEvent_t evd = nullptr;                 // after the device-to-host copy of the launch's results
    hipStream_t launch_stream = nullptr;      // stream the launches go to (= stream)
    FwPinned h_in, h_out;  // h_in = [FwSeg x ns | accepted ints]
    FwDevBuf d_in, d_out;
    FwDevBuf d_acc;  // arena of the live jobs' accepted lists (uploaded once per job, not once per round)
};

struct FwComm;  // library-side RCCL communicator state (fw_rccl.cpp)

struct fw_ctx {
    fw_params P{};
    FwComm *comm = nullptr;  // fw_comm_init: the library's own communicator for target-sharded runs
    int64_t n_obs_min_eff = 0;
    mutable std::string err;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;

    // ---- continuous (FW_FZ) ----
    float *d_data = nullptr;  // n x p column-major, as uploaded
    float *d_xc = nullptr;    // centred columns, [p_pad][n_pad], zero padded
    float *d_sd = nullptr;    // sqrt(sum xc^2) per column, [p_pad]
    float *d_cor = nullptr;   // p x p (symmetric)
    bool cor_external = false;  // d_cor is caller-owned device memory (fw_use_cor_buffer): never freed here
    int64_t cor_capacity = 0;   // ... and holds this many floats
    int cor_rows_rank = -1, cor_rows_world = 0;  // what the last fw_compute_cor_mat_rows computed: rank / world / rows per rank
    int64_t cor_rows_per_rank = 0;               // (fw_cor_mat_allgather_comm checks its arguments against them)
    double *d_thr = nullptr;  // |r| significance thresholds of the segment kernel (fz_thresholds_kernel)
    double *d_fzs_stat = nullptr;  // recursive_pcor = 0: per column {mean, sum of squared deviations in both summation orders} in Float64 (fw_fzs.hip, FZS_ST)
    uint64_t gram_epoch = 0;       // recursive_pcor = 0: bumped whenever the job-matrix arena loses its contents (new pool, reallocation, reset)
    bool have_fzs_stat = false;
    int n_pad = 0, p_pad = 0;
    bool have_data = false, have_cor = false;
    // Float64 mode (fw_set_data_dense_f64 / fw_set_cor_mat_f64, fw_fz64.hip): its own buffers, nothing of the above but d_thr is used
    bool f64 = false;       // the context is in Float64 mode
    bool f32_input = false; // a Float32 matrix was uploaded (fw_set_data_dense_f32 / fw_set_cor_mat): the mode can no longer change
    double *d_data64 = nullptr, *d_xc64 = nullptr, *d_sd64 = nullptr, *d_cor64 = nullptr;

    // ---- discrete (FW_MI / FW_MI_NZ) ----
    std::vector<int32_t> levels, max_vals;
    int L = 0;                   // maximum(max_vals) + 1
    int elim_mode = 0;  // fw_learn_opts.elim_mode of the running fw_learn_network (read by the device rounds, fw_devhiton.hip)
    int mi_view = 0;  // dense rules + mi_nz: test_subsets evaluates on the (T, candidate) row view of hiton.jl:41-50 (fw_set_row_views)
    int l0_rank = 0, l0_world = 1;  // fw_level0_sharded: this rank's share of the level-0 pair tiles (discrete kinds)
    double *d_gthr = nullptr;    // [df]: G^2 quantile with ccdf(Chisq(df), .) = alpha (significance without evaluating Q(a, x))
    int gthr_n = 0;
    int mi_nxy = 2;              // cells per stratum side of the conditional-test kernels (fw_mi_core.h): 3 only for "mi" on 3-valued data
    int W = 0;                   // 64-bit words per packed column
    uint64_t *d_nzbits = nullptr;  // [p][W] bit i of word w: sample 64w+i has value != 0
    uint64_t *d_hibits = nullptr;  // [p][W] value == 2 (second non-zero level); NULL when L == 2
    int32_t *d_levels = nullptr, *d_maxvals = nullptr;
    unsigned char *d_vals = nullptr;  // generic discrete form (a value above 2): one byte per (variable, sample), [p][n]; null otherwise
    bool mi_generic = false;
    // generic form, tables beyond the LDS of a wavefront (r05: more than 8 levels, or 4-8 levels at a max_k the LDS table does not hold):
    // one table per wavefront of a launch in device memory, launches cut so that the tables of one fit mig_gtab_bytes_max
    long long mig_gtab_words = 0;  // words of one table (0: the table lives in LDS)
    FwDevBuf d_mig_tab[3];  // [the engine's own stream, pool 0, pool 1]: two pools can be in flight
    // fz_nz, CSC-resident layout (fw_set_data_csc_f32_resident, fw_cscres.h): d_nzbits is the plane, d_data stays null
    bool csc_resident = false;
    uint32_t *d_cbase = nullptr;  // [p][W] position in d_cvals of the column's first entry at or after row 64 w
    float *d_cvals = nullptr;     // values != 0.0f, column after column, rows ascending (max(cvals_n, 1) floats)
    int64_t cvals_n = 0;
    bool fznz_lds_raised_csc = false;  // as fznz_lds_raised, for the kernel's CSC instantiation
    bool fznz_lds_raised = false;  // fznz_submat_kernel's dynamic-LDS limit was raised on this context's device (a property of (function, device): one flag per context, set under the context's own launches)
    float *d_xlnx = nullptr;       // [x ln x | ln x] for x = 0..n (Float32 tables of the discrete level-0 screen)
    int32_t *d_firstnz = nullptr;  // per column: index of the first non-zero sample (n if none)

    // ---- level-0 result (host, CSR) ----
    bool have_level0 = false;
    std::vector<int64_t> nb_off;
    std::vector<int32_t> nb_idx;
    std::vector<double> nb_stat, nb_p;

    // ---- network result ----
    bool have_network = false;
    FwHostWorkers *host_workers = nullptr;  // host threads of the graph passes (fw_graph.h), started at the first network that wants them
    FwNetwork net;

    // ---- rejection log (fw_set_track_rejections) ----
    // One slot per directed level-0 entry: the record of (T, candidate) lives at the candidate's position in T's level-0 list
    // (nb_off[T] + index of the candidate in the ascending list), n_zs = -1 while empty.  The host job pool fills rej_slots, the device
    // paths the device copy; fw_learn_network merges the two and compacts them into rej (ascending target, candidate).
    int track_rej = 0;
    bool have_rej = false;
    std::vector<fw_rejection> rej, rej_slots;
    FwDevBuf d_rej;
    fw_rejection *d_rej_run = nullptr;  // non-null while a tracked fw_learn_network runs (read by fw_devhiton.hip)
    // fw_rejections_allgather_* (fw_xchg.hip): what the last fw_learn_network left for it.  The device slots stay as the run wrote
    // them; of the host job pool's slots only the filled ones are kept, as (slot, which side wrote it) beside every entry of rej.
    size_t rej_n_last = 0;            // slots of the last run (0: it logged nothing)
    int rej_rank = 0, rej_world = 1;  // its fw_learn_opts.rank / world_size
    bool rej_gathered = false;        // rej already holds every rank's entries
    std::vector<int64_t> rej_slot;    // per entry of rej: its slot
    std::vector<uint8_t> rej_host;    // per entry of rej: 1 = written by the host job pool (not in d_rej yet)
    FwDevBuf d_rej_x;                 // counters + staging of the host-written records on their way into d_rej
    int64_t rej_packed_host = 0, rej_packed_dev = 0, rej_received = 0;  // last gather: records packed by origin, records of other ranks placed

    fw_counters cnt{};

    // grow-only scratch
    FwDevBuf d_jobs, d_acc, d_out, d_tmp0, d_tmp1, d_tmp2, d_segs, d_segout, d_nzrecs, d_arena;
    FwDevBuf d_l0m_i, d_l0m_d;  // level-0 pairs merged over the ranks (fw_xchg.hip)
    FwDevBuf d_bh;  // scratch of the device-side BH / neighbour-list epilogue (fw_bh.hip)
    // device copies of the level-0 neighbour CSR (inside d_bh, valid until the next fw_level0); null after a host-side BH
    const long long *d_nb_off = nullptr;
    const int32_t *d_nb_idx = nullptr;
    const double *d_nb_stat = nullptr, *d_nb_p = nullptr;
    const int32_t *d_cand = nullptr;  // per variable: its neighbours in candidate order (ascending adjusted p, stable)
    unsigned long long l0_cap_hint = 0;  // most screened / significant level-0 pairs seen so far (sizes the next call's buffers)
    bool nb_host_valid = true;        // nb_idx / nb_stat / nb_p hold the current lists (nb_off always does)
#define FW_DH_MAX_CHAINS 4
    FwDevBuf d_dh[FW_DH_MAX_CHAINS];  // arenas of the device-resident HITON rounds (fw_devhiton.hip), one per concurrent chain
    FwPinned h_dh[FW_DH_MAX_CHAINS];  // their pinned flag pages
    hipStream_t dh_stream[FW_DH_MAX_CHAINS] = {nullptr, nullptr, nullptr, nullptr};  // streams of chains 1.. (chain 0: pb[0].stream)
    // r06: a high-priority stream per chain for the small kernels between two segment launches (step / compact / plan / fill), with the two events
    // that tie it to the chain's stream -- used where the segment launches are long (max_k > 3): a one-workgroup kernel then no longer queues behind
    // the thousands of pending workgroups of the OTHER chain's segment kernel
    hipStream_t dh_hp_stream[FW_DH_MAX_CHAINS] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t dh_hp_ev[FW_DH_MAX_CHAINS][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    FwPinned h_jobs, h_acc, h_out;
    FwPoolBuf pb[2];
};

// Tuning / test knobs (environment variables FW_*, read ONLY when FW_KNOBS=1 is set): the list, the gate and the readers are in
// fw_knobs.h; DESIGN.md section 5 carries the same table.
#include "fw_knobs.h"

int fw_fail(const fw_ctx *ctx, int code, const char *fmt, ...);
int fw_dev_reserve(fw_ctx *ctx, FwDevBuf &b, size_t bytes);
int fw_pin_reserve(fw_ctx *ctx, FwPinned &b, size_t bytes);

#define FW_HIP(ctx, call)                                                                        \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return fw_fail(ctx, FW_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), \
                           __FILE__, __LINE__);                                                  \
    } while (0)

// FW_HIP where running out of device memory is a capacity answer (FW_ERR_NOMEM), not a device error
#define FW_HIP_MEM(ctx, call)                                                                    \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess)                                                                   \
            return fw_fail(ctx, e__ == hipErrorOutOfMemory ? FW_ERR_NOMEM : FW_ERR_DEVICE, "%s failed: %s (%s:%d)", #call, \
                           hipGetErrorString(e__), __FILE__, __LINE__);                          \
    } while (0)

// ---- a CSC triple the *_csc_*_dev entry points borrow (fw_norm.hip, fw_core.cpp): colptr[p + 1] Int64, rowval[nnz] Int32, nzval[nnz] ----
// Every pointer is asked of the runtime before anything reads it (rowval / nzval only when there are entries).
inline int fwi_csc_dev_ptrs(const fw_ctx *ctx, const char *fn, int device, const void *colptr, const void *rowval, const void *nzval, long long nnz)
{
    if (nnz < 0) return fw_fail(ctx, FW_ERR_ARG, "%s: nnz = %lld", fn, nnz);
    if (!colptr || (nnz > 0 && (!rowval || !nzval))) return fw_fail(ctx, FW_ERR_ARG, "%s: NULL array", fn);
    if (!fw_is_dev_ptr(colptr, device) || (nnz > 0 && (!fw_is_dev_ptr(rowval, device) || !fw_is_dev_ptr(nzval, device))))
        return fw_fail(ctx, FW_ERR_ARG, "%s: the triple is not device memory of device %d (the entry point without _dev takes host arrays)", fn, device);
    return FW_OK;
}
// The p + 1 column pointers, downloaded and checked before any kernel reads rowval or nzval: they run monotonically from 0 to nnz, so
// every column's range lies inside the two arrays of nnz entries.  What the kernels' own column check (fw_csc.h) would say, said first.
inline int fwi_csc_dev_colptr(const fw_ctx *ctx, const char *fn, const int64_t *d_colptr, int p, long long nnz, std::vector<int64_t> &colptr)
{
    colptr.resize((size_t)p + 1);
    FW_HIP(ctx, hipMemcpy(colptr.data(), d_colptr, sizeof(int64_t) * ((size_t)p + 1), hipMemcpyDeviceToHost));
    if (colptr[0] != 0 || colptr[p] != nnz) return fw_fail(ctx, FW_ERR_ARG, "%s: colptr must run from 0 to nnz (column 0)", fn);
    for (int j = 0; j < p; ++j)
        if (colptr[j + 1] < colptr[j]) return fw_fail(ctx, FW_ERR_ARG, "%s: column %d: colptr is not monotone within 0 .. nnz", fn, j);
    return FW_OK;
}

// ---- what the kinds' back-ends share (fw_core.cpp; the capacity policy itself: fw_stage_host.h) ----
// The attempts of a level-0 driver on the context's hint; run(cap, counts) is one attempt, `what` names the buffer in the error.
template <class Run> int fwi_l0_attempts(fw_ctx *ctx, long long pairs, long long limit, const char *what, Run &&run)
{
    std::string overflow;
    const int rc = fw_l0_attempts(fw_l0_first_cap(pairs, limit, ctx->l0_cap_hint), ctx->l0_cap_hint, what, overflow, run);
    return overflow.empty() ? rc : fw_fail(ctx, rc, "%s", overflow.c_str());
}
// The k significant pairs of a level-0 driver, handed over: left where they are for fwi_bh_csr_device (dev != null; the vectors end
// empty) or downloaded into the vectors.  The statistic is Float64 (stat64) or Float32 (stat32, widened on the host), the other null.
int fwi_l0_handover(fw_ctx *ctx, const int32_t *oi, const int32_t *oj, const double *stat64, const float *stat32, const double *op, size_t k,
                    std::vector<int32_t> &pi, std::vector<int32_t> &pj, std::vector<double> &stat, std::vector<double> &pval, FwL0Dev *dev);
// Staging of an explicit-test batch (fw_test_batch) on ctx->stream: zoff | X | Y in ctx->d_jobs, zflat in ctx->d_acc, room for the m
// results in ctx->d_out.  fwi_batch_finish after the launches: launch error, results to `out`, synchronise, count the batch.
struct FwBatch {
    long long *dz = nullptr;
    int32_t *dX = nullptr, *dY = nullptr;
    const int32_t *dzflat = nullptr;
    fw_test_result *dout = nullptr;
    int kmax = 0;  // the batch's largest conditioning set
};
int fwi_batch_upload(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff, const int32_t *zflat, FwBatch &b);
int fwi_batch_finish(fw_ctx *ctx, int64_t m, fw_test_result *out);
void fw_fill_no_power(fw_test_result *out, int64_t m);  // tests.jl:11 / :254: too few observations, every test {0, 1, 0, 0}

// ---- fz (fw_fz.hip) ----
int fwi_fz_compute_cor(fw_ctx *ctx);
int fwi_fz_compute_cor_rows(fw_ctx *ctx, int rank, int world, int64_t *row0, int64_t *rows_per_rank);
int fwi_fz_level0(fw_ctx *ctx, std::vector<int32_t> &pi, std::vector<int32_t> &pj, std::vector<double> &stat,
                  std::vector<double> &pval, int64_t *m_reliable, FwL0Dev *dev);
int fwi_fz_test_batch(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff,
                      const int32_t *zflat, fw_test_result *out);
int fwi_fz_segments(fw_ctx *ctx, int64_t nseg, int64_t nseg_tab, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, FwPoolBuf &pb);

// ---- fz in Float64 (fw_fz64.hip): the context's f64 mode ----
int fwi_fz64_set_data(fw_ctx *ctx, const double *data);
int fwi_fz64_set_cor(fw_ctx *ctx, const double *cor);
int fwi_fz64_get_cor(const fw_ctx *ctx, double *out);
int fwi_fz64_compute_cor(fw_ctx *ctx);
int fwi_fz64_level0(fw_ctx *ctx, std::vector<int32_t> &pi, std::vector<int32_t> &pj, std::vector<double> &stat, std::vector<double> &pval,
                    int64_t *m_reliable, FwL0Dev *dev);
int fwi_fz64_test_batch(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff, const int32_t *zflat,
                        fw_test_result *out);
int fwi_fz64_segments(fw_ctx *ctx, int64_t nseg, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, FwPoolBuf &pb);

// ---- fz without a correlation matrix: streamed sample columns (fw_fzs.hip, fw_params.recursive_pcor = 0) ----
int fwi_fzs_test_batch(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff, const int32_t *zflat,
                       fw_test_result *out);
int fwi_fzs_segments(fw_ctx *ctx, int64_t nseg, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, FwPoolBuf &pb,
                     const FwNzJob *recs_host, int64_t njobs, size_t arena_doubles);
int fwi_fzs_segments_nz(fw_ctx *ctx, int64_t nseg, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, FwPoolBuf &pb, int m_max);  // fz_nz, recursive_pcor = 0  // recs: one per launched job (FwSeg::pad indexes them); rec.nR != 0: matrix to be computed

// ---- HE-S / fz_nz (fw_fz.hip) ----
int fwi_fznz_upload(fw_ctx *ctx, const float *data);
int fwi_fznz_upload_dev(fw_ctx *ctx, const float *d_src);  // the same layout from a [p][n] matrix in device memory: copy + plane kernel
int fwi_fznz_upload_csc(fw_ctx *ctx, const int64_t *colptr, const int32_t *rowval, const float *nzval);  // the same layout from a CSC triple
int fwi_fznz_upload_csc_resident(fw_ctx *ctx, const int64_t *colptr, const int32_t *rowval, const float *nzval);  // plane + base + values != 0 (fw_cscres.h)
// the two CSC uploads on a triple that lies in device memory (pointers and column pointers checked by the entry point): nothing is staged
int fwi_fznz_upload_csc_dev(fw_ctx *ctx, const int64_t *d_colptr, const int32_t *d_rowval, const float *d_nzval, long long nnz);
int fwi_fznz_upload_csc_resident_dev(fw_ctx *ctx, const int64_t *d_colptr, const int32_t *d_rowval, const float *d_nzval, long long nnz);
int fwi_fznz_level0(fw_ctx *ctx, std::vector<int32_t> &pi, std::vector<int32_t> &pj, std::vector<double> &stat,
                    std::vector<double> &pval, int64_t *m_reliable, FwL0Dev *dev);
int fwi_fznz_submatrices(fw_ctx *ctx, int64_t njobs, const FwNzJob *recs_host, size_t arena_floats, const int32_t *d_acc,
                         hipStream_t stream, bool f64 = false);
void fwi_host_workers_free(fw_ctx *c);
#ifdef FW_FZ_FASTDBG
extern "C" void fwi_fz_fastdbg_print();  // fw_fz.hip: counters of the size-3 fast loop (profiling build only)
#endif
int fwi_mi_big_limits(fw_ctx *ctx, int k);  // FW_OK if discrete tests with k (6, 7) conditioning variables fit the large LDS table
int fwi_fznz_dev_limits(fw_ctx *ctx, int m_max);  // FW_OK if a job of m_max variables fits the sub-matrix kernel's LDS
int fwi_fznz_submatrices_dev(fw_ctx *ctx, int nslots, FwNzJob *d_recs, const int32_t *d_acc, float *d_arena, int m_max, bool any_long, hipStream_t stream);
int fwi_fznz_segments_dev(fw_ctx *ctx, unsigned grid, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, const unsigned *d_ns,
                          bool any_big, const unsigned *d_big, const FwNzJob *d_recs, const float *d_arena, hipStream_t stream);
int fwi_fznz_segments(fw_ctx *ctx, int64_t nseg, int64_t nseg_tab, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, FwPoolBuf &pb);
int fwi_fznz_test_batch(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff,
                        const int32_t *zflat, fw_test_result *out);

// ---- discrete (fw_mi.hip) ----
int fwi_mi_upload(fw_ctx *ctx, const int64_t *colptr, const int32_t *rowval, const int32_t *nzval);
int fwi_mi_upload_dev(fw_ctx *ctx, const int32_t *d_src);  // the same layouts from a [p][n] table in device memory: column scan + pack
int fwi_mi_upload_csc_dev(fw_ctx *ctx, const int64_t *d_colptr, const int32_t *d_rowval, const int32_t *d_nzval, long long nnz);  // ... from a CSC triple in device memory
int fwi_mi_level0(fw_ctx *ctx, std::vector<int32_t> &pi, std::vector<int32_t> &pj, std::vector<double> &stat,
                  std::vector<double> &pval, int64_t *m_reliable, FwL0Dev *dev);
int fwi_mi_test_batch(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff,
                      const int32_t *zflat, fw_test_result *out);
int fwi_mi_segments(fw_ctx *ctx, int64_t nseg, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, FwPoolBuf &pb);

// algorithmic bytes of the first `evaluated` tests of a job with |accepted| = a (enumeration order: sizes max_k..1)
double fwi_alg_bytes(const fw_ctx *ctx, int a, int64_t evaluated);

// ---- asynchronous job pool (fw_pool.cpp; records and rules: fw_pool_host.h): every round evaluates one window of every live job in ONE launch ----
struct FwPoolJob : FwJobRun {
    int32_t X = 0, Y = 0;
    int64_t tag = 0;     // caller's id (driver: target slot)
    int32_t aux = 0;     // driver: candidate index
    int32_t epoch = 0;   // driver: accepted-set epoch of the owner when the job was posted (stale jobs are dropped)
    bool hold = false;     // driver: do not launch further windows for now (speculative job past its first window)
    bool launched = false; // set by fwi_pool_launch for the jobs that are part of the pending window
    std::vector<int32_t> acc;
    int64_t acc_dev_off = -1;  // offset (ints) of this job's accepted list in the pool buffer's device arena, -1 = not uploaded
    int64_t gram_off = -1;     // recursive_pcor = 0: offset (doubles) of the job's correlation matrix in ctx->d_arena, valid while
    uint64_t gram_epoch = 0;   // ... gram_epoch == ctx->gram_epoch (the arena was neither reallocated nor reset since)
    int32_t rec = -1;          // fz_nz, recursive_pcor = 0: index of the job's record in pool.nzrecs of the pending launch
};
struct FwPool {
    std::vector<FwPoolJob> live;
    std::vector<int64_t> seg_job;
    std::vector<FwNzJob> nzrecs;  // fz_nz: job records of the pending launch
    int buf = 0;            // which ctx->pb[] this pool stages through
    bool want_zs = false;   // recover the conditioning set of each returned result from its rank (ABI path)
    const std::vector<int32_t> *owner_epoch = nullptr;  // if set: jobs whose epoch != (*owner_epoch)[tag] are cancelled
    int64_t dropped_evaluated = 0;                      // tests already evaluated for jobs cancelled before they finished
    double dropped_alg_bytes = 0.0;
    bool inflight = false;  // a window launch is pending (fwi_pool_launch without fwi_pool_collect)
    size_t ns = 0;
    uint64_t launched_ranks = 0;  // ranks of the pending / last launch (window-growth policy)
    size_t arena_top = 0;         // ints used in pb.d_acc (accepted lists stay resident while their job lives)
    size_t gram_top = 0;          // recursive_pcor = 0: doubles used in ctx->d_arena by this pool's job matrices (kept across rounds)
    uint64_t gram_epoch = 0;      // epoch of ctx->d_arena this pool's offsets belong to (0: none yet)
    double t_launch = 0.0;
};
int fwi_pool_launch(fw_ctx *ctx, FwPool &pool);                                    // asynchronous
int fwi_pool_collect(fw_ctx *ctx, FwPool &pool, std::vector<FwPoolJob> &finished);  // waits + merges
int fwi_pool_add(fw_ctx *ctx, FwPool &pool, int32_t X, int32_t Y, const int32_t *acc, int a, int64_t tag);
int fwi_pool_round(fw_ctx *ctx, FwPool &pool, std::vector<FwPoolJob> &finished);

// device-side Benjamini-Hochberg + neighbour CSR (fw_bh.hip); fills ctx->nb_off / nb_idx / nb_stat / nb_p
int fwi_bh_csr_device(fw_ctx *ctx, const FwL0Dev &in, int64_t m_reliable);
// device-resident all-gather of the ranks' significant level-0 pairs (fw_xchg.hip)
int fwi_l0_exchange_dev(fw_ctx *c, const fw_dev_exchange *x, int world, const FwL0Dev &local, int64_t m_local, FwL0Dev *merged, int64_t *m_sum);
// all-gather of the ranks' rejection logs through a fw_dev_exchange (fw_xchg.hip); `who` names the entry point in messages
int fwi_rej_allgather(fw_ctx *c, const fw_dev_exchange *x, const char *who);
// fw_hiton.cpp: slot array in device memory (+ host_slots, may be null: the job pool's) -> ctx->rej, ascending (target, candidate)
int fwi_rej_compact(fw_ctx *c, size_t rej_n, const fw_rejection *host_slots);
int fwi_selftest_div(fw_ctx *ctx, unsigned long long cases, unsigned long long seed, unsigned long long *mismatches);  // fw_fz.hip
void fwi_comm_free(fw_ctx *ctx);  // fw_rccl.cpp
int fwi_nb_host_ensure(fw_ctx *ctx);  // download partners / statistics / adjusted p if only the device holds them

// ---- device-resident HITON rounds (fw_devhiton.hip, FW_FZ) ----
struct FwDhTarget {
    int32_t T = 0;
    std::vector<int32_t> cands;  // interleaving candidates in hiton.jl:211-217 order (unused when nc_dev >= 0)
    int32_t nc_dev = -1;         // >= 0: take the first nc_dev entries of ctx->d_cand at nb_off[T] (device-built order)
    const int32_t *wl = nullptr; // sorted whitelist (feed-forward), may be null
    int wl_n = 0;
};
struct FwDhResult {  // PC of one target in insertion order: entries [off, off + n) of the run's flat arrays
    int64_t off = 0;
    int32_t n = 0;
};
struct FwDhFlat {  // (one allocation per run instead of three per target: 150 000 small vectors were 10 ms of a cfg4 pass)
    std::vector<int32_t> key;
    std::vector<double> stat, pval;
};
int fwi_devhiton_run(fw_ctx *ctx, const std::vector<FwDhTarget> &in, std::vector<FwDhResult> &out, FwDhFlat &flat, int chain = 0);
// the whole feed-forward schedule of the discrete kinds on the device: whitelists built between the launches, one download (r05)
int fwi_devhiton_mi_schedule(fw_ctx *ctx, const int32_t *sched, int nt, int R, bool feed_forward, FwDirected &all);
// the same for Fisher-z (device rounds on concurrent chains, the host between the rounds of targets gone)
int fwi_devhiton_fz_schedule(fw_ctx *ctx, const int32_t *sched, int nt, int R, bool feed_forward, FwDirected &all);
// fw_hiton.cpp: chains of a round of n targets, and which chain target i goes to (and its index there)
int fwi_chain_count(const fw_ctx *ctx, size_t n_targets);
void fwi_deal_chains(size_t n, int K, std::vector<int> &chain_of, std::vector<size_t> &chain_idx);
int fwi_mi_segments_dev(fw_ctx *ctx, unsigned grid, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, const unsigned *d_ns,
                        hipStream_t stream);
int fwi_fz_thresholds(fw_ctx *ctx, hipStream_t stream, double *zscale);  // ensures ctx->d_thr (fz_thresholds_kernel)
int fwi_fz_segments_dev(fw_ctx *ctx, unsigned grid, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, const unsigned *d_ns,
                        bool any_big, const unsigned *d_big, hipStream_t stream);

// ---- test_subsets batches through the job pool (fw_pool.cpp) ----
int fwi_subsets_dispatch(fw_ctx *ctx, int64_t m, const FwJob *jobs_host, const int32_t *acc_host, int64_t acc_total,
                         FwJobOut *out_host);
