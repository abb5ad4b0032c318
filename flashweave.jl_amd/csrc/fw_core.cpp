// Context lifecycle, data hand-over, the staged level 0 (host-only pieces: fw_level0_host.h), the per-pair and per-job batch entry
// points and the rest of the extern "C" surface of include/flashweave_amd.h.  Device work lives in fw_fz.hip / fw_mi.hip, the host job
// pool in fw_pool.cpp, the HITON-PC host driver in fw_hiton.cpp.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <numeric>

#include <mutex>

#include "fw_internal.h"
#include "fw_level0_host.h"

static thread_local std::string g_create_err;

int fw_fail(const fw_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) {
        // concurrent device-HITON chains (fw_hiton.cpp, one host thread each) may fail at the same time: the message is
        // a std::string, so writers are serialised; the first message of a call wins (fw_learn_network clears it)
        static std::mutex err_mu;
        std::lock_guard<std::mutex> lk(err_mu);
        ctx->err = buf;
    } else {
        g_create_err = buf;
    }
    return code;
}

int fw_dev_reserve(fw_ctx *ctx, FwDevBuf &b, size_t bytes)
{
    if (bytes <= b.cap) return FW_OK;
    if (b.ptr) FW_HIP(ctx, hipFree(b.ptr));
    b.ptr = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 2 + 256;
    hipError_t e = hipMalloc(&b.ptr, want);
    if (e != hipSuccess) return fw_fail(ctx, FW_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    b.cap = want;
    return FW_OK;
}

int fw_pin_reserve(fw_ctx *ctx, FwPinned &b, size_t bytes)
{
    if (bytes <= b.cap) return FW_OK;
    if (b.ptr) FW_HIP(ctx, hipHostFree(b.ptr));
    b.ptr = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 2 + 256;
    hipError_t e = hipHostMalloc(&b.ptr, want, hipHostMallocDefault);
    if (e != hipSuccess) return fw_fail(ctx, FW_ERR_NOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    b.cap = want;
    return FW_OK;
}

int fwi_l0_handover(fw_ctx *ctx, const int32_t *oi, const int32_t *oj, const double *stat64, const float *stat32, const double *op, size_t k,
                    std::vector<int32_t> &pi, std::vector<int32_t> &pj, std::vector<double> &stat, std::vector<double> &pval, FwL0Dev *dev)
{
    pi.assign(dev ? 0 : k, 0);
    pj.assign(pi.size(), 0);
    stat.assign(pi.size(), 0.0);
    pval.assign(pi.size(), 0.0);
    if (dev) {  // results stay on the device for fwi_bh_csr_device
        *dev = FwL0Dev{oi, oj, stat64, stat32, op, k};
        return FW_OK;
    }
    if (k == 0) return FW_OK;
    std::vector<float> rr(stat32 ? k : 0);
    FW_HIP(ctx, hipMemcpy(pi.data(), oi, k * sizeof(int32_t), hipMemcpyDeviceToHost));
    FW_HIP(ctx, hipMemcpy(pj.data(), oj, k * sizeof(int32_t), hipMemcpyDeviceToHost));
    FW_HIP(ctx, stat32 ? hipMemcpy(rr.data(), stat32, k * sizeof(float), hipMemcpyDeviceToHost)
                       : hipMemcpy(stat.data(), stat64, k * sizeof(double), hipMemcpyDeviceToHost));
    FW_HIP(ctx, hipMemcpy(pval.data(), op, k * sizeof(double), hipMemcpyDeviceToHost));
    if (stat32) std::copy(rr.begin(), rr.end(), stat.begin());
    return FW_OK;
}

int fwi_batch_upload(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff, const int32_t *zflat, FwBatch &b)
{
    const int64_t nz = zoff[m];
    int rc;
    if ((rc = fw_dev_reserve(ctx, ctx->d_jobs, (size_t)m * 2 * sizeof(int32_t) + (size_t)(m + 1) * sizeof(int64_t)))) return rc;
    if ((rc = fw_dev_reserve(ctx, ctx->d_acc, (size_t)(nz > 0 ? nz : 1) * sizeof(int32_t)))) return rc;
    if ((rc = fw_dev_reserve(ctx, ctx->d_out, (size_t)m * sizeof(fw_test_result)))) return rc;
    b.dz = (long long *)ctx->d_jobs.ptr;
    b.dX = (int32_t *)(b.dz + m + 1);
    b.dY = b.dX + m;
    b.dzflat = (const int32_t *)ctx->d_acc.ptr;
    b.dout = (fw_test_result *)ctx->d_out.ptr;
    FW_HIP(ctx, hipMemcpyAsync(b.dz, zoff, (size_t)(m + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
    FW_HIP(ctx, hipMemcpyAsync(b.dX, X, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    FW_HIP(ctx, hipMemcpyAsync(b.dY, Y, (size_t)m * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    if (nz > 0) FW_HIP(ctx, hipMemcpyAsync(ctx->d_acc.ptr, zflat, (size_t)nz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    b.kmax = 0;
    for (int64_t t = 0; t < m; ++t) b.kmax = std::max<int>(b.kmax, (int)(zoff[t + 1] - zoff[t]));
    return FW_OK;
}

int fwi_batch_finish(fw_ctx *ctx, int64_t m, fw_test_result *out)
{
    FW_HIP(ctx, hipGetLastError());
    FW_HIP(ctx, hipMemcpyAsync(out, ctx->d_out.ptr, (size_t)m * sizeof(fw_test_result), hipMemcpyDeviceToHost, ctx->stream));
    FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cnt.kernel_launches += 1;
    return FW_OK;
}

void fw_fill_no_power(fw_test_result *out, int64_t m)
{
    for (int64_t t = 0; t < m; ++t) out[t] = fw_test_result{0.0, 1.0, 0, 0};
}

extern "C" {

int fw_abi_version(void) { return FW_ABI_VERSION; }

void fw_params_default(fw_params *P, int32_t kind, int32_t n, int32_t p)
{
    if (!P) return;
    memset(P, 0, sizeof(*P));
    P->kind = kind;
    P->n = n;
    P->p = p;
    P->device = 0;
    P->max_k = 3;
    P->hps = 5;
    P->fdr = 1;
    P->n_obs_min = -1;
    P->max_tests = 10000000;
    P->alpha = 0.01;
    P->recursive_pcor = 1;
}

const char *fw_last_error(const fw_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int fw_ctx_create(const fw_params *P, fw_ctx **out)
{
    if (out) *out = nullptr;
    if (!P || !out) return fw_fail(nullptr, FW_ERR_ARG, "fw_ctx_create: NULL argument");
    if (P->kind != FW_MI && P->kind != FW_MI_NZ && P->kind != FW_FZ && P->kind != FW_FZ_NZ)
        return fw_fail(nullptr, FW_ERR_ARG, "fw_ctx_create: unknown test kind %d", P->kind);
    if (P->n <= 0 || P->p <= 1) return fw_fail(nullptr, FW_ERR_ARG, "fw_ctx_create: need n > 0 and p > 1 (n=%d, p=%d)", P->n, P->p);
    if (P->max_k < 0 || P->max_k > FW_MAX_K)
        return fw_fail(nullptr, FW_ERR_LIMIT, "fw_ctx_create: max_k=%d outside [0, %d]", P->max_k, FW_MAX_K);
    if (P->max_k > FW_MAX_K_FAST && (P->kind == FW_FZ || P->kind == FW_FZ_NZ) && !P->recursive_pcor)
        return fw_fail(nullptr, FW_ERR_LIMIT, "fw_ctx_create: max_k=%d with recursive_pcor = 0 (conditioning on job-local Gram matrices serves max_k <= %d)",
                       P->max_k, FW_MAX_K_FAST);
    if (!(P->alpha > 0.0 && P->alpha < 1.0)) return fw_fail(nullptr, FW_ERR_ARG, "fw_ctx_create: alpha must be in (0,1)");
    if (P->hps < 0) return fw_fail(nullptr, FW_ERR_ARG, "fw_ctx_create: hps must be >= 0");
    if (P->dense_rules && (P->kind == FW_FZ || P->kind == FW_FZ_NZ))
        return fw_fail(nullptr, FW_ERR_ARG, "fw_ctx_create: dense_rules applies to the discrete tests only");
    if (P->no_cor_mat && (P->kind != FW_FZ || P->recursive_pcor))
        return fw_fail(nullptr, FW_ERR_ARG, "fw_ctx_create: no_cor_mat (dense_cor = false) needs FW_FZ with recursive_pcor = 0 "
                                            "(without a matrix the conditional tests come from the data, tests.jl:253)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fw_fail(nullptr, FW_ERR_DEVICE, "fw_ctx_create: no HIP device available (%s); this engine has no CPU fallback",
                       e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (P->device < 0 || P->device >= ndev)
        return fw_fail(nullptr, FW_ERR_DEVICE, "fw_ctx_create: device %d out of range (have %d)", P->device, ndev);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, P->device)) != hipSuccess)
        return fw_fail(nullptr, FW_ERR_DEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fw_fail(nullptr, FW_ERR_DEVICE, "fw_ctx_create: device %d is %s; kernels are built for gfx950 only", P->device,
                       prop.gcnArchName);
    if ((e = hipSetDevice(P->device)) != hipSuccess) return fw_fail(nullptr, FW_ERR_DEVICE, "hipSetDevice: %s", hipGetErrorString(e));
    fw_ctx *c = new (std::nothrow) fw_ctx();
    if (!c) return fw_fail(nullptr, FW_ERR_NOMEM, "out of host memory");
    c->P = *P;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&c->ev0)) != hipSuccess || (e = hipEventCreate(&c->ev1)) != hipSuccess) {
        delete c;
        return fw_fail(nullptr, FW_ERR_DEVICE, "stream/event creation failed: %s", hipGetErrorString(e));
    }
    for (FwPoolBuf &b : c->pb)
        if ((e = hipStreamCreateWithFlags(&b.stream, hipStreamNonBlocking)) != hipSuccess ||
            (e = hipEventCreate(&b.ev0)) != hipSuccess || (e = hipEventCreate(&b.ev1)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&b.evd, hipEventDisableTiming)) != hipSuccess) {
            fw_ctx_destroy(c);
            return fw_fail(nullptr, FW_ERR_DEVICE, "stream/event creation failed: %s", hipGetErrorString(e));
        }
    for (FwPoolBuf &b : c->pb) b.launch_stream = b.stream;
    // continuous: the automatic n_obs_min is known immediately (learning.jl:59-61); discrete needs levels
    c->n_obs_min_eff = P->n_obs_min >= 0 ? P->n_obs_min : ((P->kind == FW_FZ || P->kind == FW_FZ_NZ) ? 20 : -1);
    *out = c;
    return FW_OK;
}

static void free_dev(FwDevBuf &b)
{
    if (b.ptr) (void)hipFree(b.ptr);
    b.ptr = nullptr;
    b.cap = 0;
}
static void free_pin(FwPinned &b)
{
    if (b.ptr) (void)hipHostFree(b.ptr);
    b.ptr = nullptr;
    b.cap = 0;
}

int fw_ctx_destroy(fw_ctx *c)
{
    if (!c) return FW_OK;
    (void)hipSetDevice(c->P.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    fwi_comm_free(c);
    fwi_host_workers_free(c);
#ifdef FW_FZ_FASTDBG
    fwi_fz_fastdbg_print();
#endif
    if (c->cor_external) c->d_cor = nullptr;  // caller-owned (fw_use_cor_buffer)
    void *ptrs[] = {c->d_data64, c->d_xc64, c->d_sd64, c->d_cor64, c->d_data, c->d_xc, c->d_sd, c->d_cor, c->d_thr, c->d_fzs_stat, c->d_nzbits, c->d_hibits, c->d_levels, c->d_maxvals, c->d_firstnz, c->d_xlnx, c->d_gthr, c->d_vals, c->d_cbase, c->d_cvals};
    for (void *q : ptrs)
        if (q) (void)hipFree(q);
    free_dev(c->d_jobs);
    free_dev(c->d_acc);
    free_dev(c->d_out);
    free_dev(c->d_tmp0);
    free_dev(c->d_tmp1);
    free_dev(c->d_tmp2);
    free_dev(c->d_segs);
    free_dev(c->d_segout);
    free_dev(c->d_nzrecs);
    free_dev(c->d_arena);
    free_dev(c->d_bh);
    free_dev(c->d_rej);
    free_dev(c->d_rej_x);
    free_dev(c->d_l0m_i);
    free_dev(c->d_l0m_d);
    for (FwDevBuf &b : c->d_mig_tab) free_dev(b);
    for (int q = 0; q < FW_DH_MAX_CHAINS; ++q) {
        free_dev(c->d_dh[q]);
        free_pin(c->h_dh[q]);
        if (c->dh_stream[q]) (void)hipStreamDestroy(c->dh_stream[q]);
        if (c->dh_hp_stream[q]) (void)hipStreamDestroy(c->dh_hp_stream[q]);
        for (int e = 0; e < 2; ++e)
            if (c->dh_hp_ev[q][e]) (void)hipEventDestroy(c->dh_hp_ev[q][e]);
    }
    free_pin(c->h_jobs);
    free_pin(c->h_acc);
    free_pin(c->h_out);
    for (FwPoolBuf &b : c->pb) {
        if (b.stream) (void)hipStreamSynchronize(b.stream);
        free_pin(b.h_in);
        free_pin(b.h_out);
        free_dev(b.d_in);
        free_dev(b.d_out);
        free_dev(b.d_acc);
        if (b.ev0) (void)hipEventDestroy(b.ev0);
        if (b.ev1) (void)hipEventDestroy(b.ev1);
        if (b.evd) (void)hipEventDestroy(b.evd);
        if (b.stream) (void)hipStreamDestroy(b.stream);
    }
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return FW_OK;
}

#define CHECK_CTX(c)                                          \
    do {                                                      \
        if (!(c)) return fw_fail(nullptr, FW_ERR_ARG, "NULL context"); \
        (void)hipSetDevice((c)->P.device);                    \
    } while (0)

int fw_set_data_dense_f32(fw_ctx *c, const float *data)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ && c->P.kind != FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_f32: context is not FW_FZ / FW_FZ_NZ");
    if (!data) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_f32: NULL data");
    if (c->f64) return fw_fail(c, FW_ERR_STATE, "fw_set_data_dense_f32: the context is in Float64 mode (fw_set_data_dense_f64 / fw_set_cor_mat_f64 came first); precisions do not mix");
    if (c->P.kind == FW_FZ_NZ) {
        int rc = fwi_fznz_upload(c, data);
        if (rc) return rc;
        c->have_data = true;
        c->have_level0 = false;
        c->have_network = false;
        return FW_OK;
    }
    const size_t bytes = sizeof(float) * (size_t)c->P.n * c->P.p;
    if (!c->d_data) FW_HIP(c, hipMalloc(&c->d_data, bytes));
    FW_HIP(c, hipMemcpy(c->d_data, data, bytes, hipMemcpyHostToDevice));
    c->f32_input = true;
    c->have_data = true;
    c->have_fzs_stat = false;
    c->have_cor = false;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_set_cor_mat(fw_ctx *c, const float *cor)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ) return fw_fail(c, FW_ERR_ARG, "fw_set_cor_mat: context is not FW_FZ");
    if (c->P.no_cor_mat) return fw_fail(c, FW_ERR_STATE, "fw_set_cor_mat: the context was created with no_cor_mat (dense_cor = false)");
    if (!cor) return fw_fail(c, FW_ERR_ARG, "fw_set_cor_mat: NULL matrix");
    if (c->f64) return fw_fail(c, FW_ERR_STATE, "fw_set_cor_mat: the context is in Float64 mode (fw_set_cor_mat_f64 takes its matrix); precisions do not mix");
    const size_t cells = (size_t)c->P.p * c->P.p, bytes = sizeof(float) * cells;
    // the device arithmetic relies on |entries| <= 1 (what cor() produces, cov2cor clamps); NaN is allowed and propagates
    for (size_t t = 0; t < cells; ++t)
        if (std::fabs(cor[t]) > 1.0f)
            return fw_fail(c, FW_ERR_ARG, "fw_set_cor_mat: entry %zu = %g is outside [-1, 1]: not a correlation matrix", t,
                           (double)cor[t]);
    if (!c->d_cor) FW_HIP(c, hipMalloc(&c->d_cor, bytes));
    FW_HIP(c, hipMemcpy(c->d_cor, cor, bytes, hipMemcpyHostToDevice));
    c->f32_input = true;
    c->have_cor = true;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_compute_cor_mat(fw_ctx *c)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ) return fw_fail(c, FW_ERR_ARG, "fw_compute_cor_mat: context is not FW_FZ");
    if (c->P.no_cor_mat) return fw_fail(c, FW_ERR_STATE, "fw_compute_cor_mat: the context was created with no_cor_mat (dense_cor = false)");
    return c->f64 ? fwi_fz64_compute_cor(c) : fwi_fz_compute_cor(c);
}

// ---- Float64 mode (learn_network(prec = 64): cont_type = Float64, learning.jl:42-45) ----
// The first Float64 upload puts an FW_FZ context in Float64 mode; what the mode does not serve is refused here, by name.
static int enter_f64(fw_ctx *c, const char *fn)
{
    if (c->P.kind != FW_FZ) return fw_fail(c, FW_ERR_ARG, "%s: context is not FW_FZ (Float64 inputs are served for the plain Fisher-z test only)", fn);
    if (c->f64) return FW_OK;
    if (c->f32_input)
        return fw_fail(c, FW_ERR_STATE, "%s: the context already holds Float32 input (fw_set_data_dense_f32 / fw_set_cor_mat); precisions do not mix", fn);
    if (c->cor_external) return fw_fail(c, FW_ERR_LIMIT, "%s: fw_use_cor_buffer (row-block sharding of the matrix) is not served in Float64 mode", fn);
    if (c->comm) return fw_fail(c, FW_ERR_LIMIT, "%s: fw_comm_init (library-side collectives) is not served in Float64 mode", fn);
    if (c->P.no_cor_mat) return fw_fail(c, FW_ERR_LIMIT, "%s: no_cor_mat = 1 (dense_cor = false) is not served in Float64 mode", fn);
    if (!c->P.recursive_pcor) return fw_fail(c, FW_ERR_LIMIT, "%s: recursive_pcor = 0 is not served in Float64 mode", fn);
    if (c->P.max_k > FW_MAX_K_FAST)
        return fw_fail(c, FW_ERR_LIMIT, "%s: max_k = %d is not served in Float64 mode (max_k <= %d)", fn, c->P.max_k, FW_MAX_K_FAST);
    c->f64 = true;
    return FW_OK;
}

int fw_set_data_dense_f64(fw_ctx *c, const double *data)
{
    CHECK_CTX(c);
    if (int rc = enter_f64(c, "fw_set_data_dense_f64")) return rc;
    if (!data) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_f64: NULL data");
    if (int rc = fwi_fz64_set_data(c, data)) return rc;
    c->have_data = true;
    c->have_cor = false;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_set_cor_mat_f64(fw_ctx *c, const double *cor)
{
    CHECK_CTX(c);
    if (int rc = enter_f64(c, "fw_set_cor_mat_f64")) return rc;
    if (!cor) return fw_fail(c, FW_ERR_ARG, "fw_set_cor_mat_f64: NULL matrix");
    const size_t cells = (size_t)c->P.p * c->P.p;
    for (size_t t = 0; t < cells; ++t)  // (as fw_set_cor_mat: NaN is allowed and propagates)
        if (std::fabs(cor[t]) > 1.0)
            return fw_fail(c, FW_ERR_ARG, "fw_set_cor_mat_f64: entry %zu = %g is outside [-1, 1]: not a correlation matrix", t, cor[t]);
    if (int rc = fwi_fz64_set_cor(c, cor)) return rc;
    c->have_cor = true;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_get_cor_mat_f64(const fw_ctx *c, double *out)
{
    CHECK_CTX(c);
    if (!c->f64) return fw_fail(c, FW_ERR_STATE, "fw_get_cor_mat_f64: the context is not in Float64 mode (fw_get_cor_mat returns its Float32 matrix)");
    if (!c->have_cor) return fw_fail(c, FW_ERR_STATE, "fw_get_cor_mat_f64: no correlation matrix resident");
    if (!out) return fw_fail(c, FW_ERR_ARG, "fw_get_cor_mat_f64: NULL output");
    return fwi_fz64_get_cor(c, out);
}

int fw_get_cor_mat(const fw_ctx *c, float *out)
{
    CHECK_CTX(c);
    if (c->f64) return fw_fail(c, FW_ERR_STATE, "fw_get_cor_mat: the context is in Float64 mode (fw_get_cor_mat_f64 returns its matrix; nothing is cast)");
    if (!c->have_cor) return fw_fail(c, FW_ERR_STATE, "fw_get_cor_mat: no correlation matrix resident");
    if (!out) return fw_fail(c, FW_ERR_ARG, "fw_get_cor_mat: NULL output");
    FW_HIP(c, hipMemcpy(out, c->d_cor, sizeof(float) * (size_t)c->P.p * c->P.p, hipMemcpyDeviceToHost));
    return FW_OK;
}

// learning.jl:51-64 automatic n_obs_min for discrete tests (needs maximum(levels))
static void resolve_n_obs_min_discrete(fw_ctx *c)
{
    if (c->P.n_obs_min >= 0) {
        c->n_obs_min_eff = c->P.n_obs_min;
        return;
    }
    int64_t max_level = 0;
    for (int32_t l : c->levels) max_level = std::max<int64_t>(max_level, l);
    int64_t n_strata = 1;
    for (int j = 0; j < c->P.max_k; ++j) {
        n_strata *= max_level;
        if (n_strata > 8) break;
    }
    n_strata = std::min<int64_t>(n_strata, 8);
    c->n_obs_min_eff = (int64_t)c->P.hps * 2 * 2 * n_strata;
}

int fw_set_data_csc_i32(fw_ctx *c, const int64_t *colptr, const int32_t *rowval, const int32_t *nzval)
{
    CHECK_CTX(c);
    if (c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_i32: context is not discrete");
    if (!colptr || (colptr[c->P.p] > 0 && (!rowval || !nzval))) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_i32: NULL array");
    int rc = fwi_mi_upload(c, colptr, rowval, nzval);
    if (rc) return rc;
    resolve_n_obs_min_discrete(c);
    c->have_data = true;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_set_data_csc_f32(fw_ctx *c, const int64_t *colptr, const int32_t *rowval, const float *nzval)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_f32: context is not FW_FZ_NZ");
    if (!colptr || (colptr[c->P.p] > 0 && (!rowval || !nzval))) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_f32: NULL array");
    c->have_data = false;  // (a refused triple leaves the resident layout half written)
    c->have_level0 = false;
    c->have_network = false;
    int rc = fwi_fznz_upload_csc(c, colptr, rowval, nzval);
    if (rc) return rc;
    c->have_data = true;
    return FW_OK;
}

// A refused triple leaves the data, the level-0 lists and the network of the context as they were.  The upload stages the triple in
// d_tmp1 and the scan's scratch in d_tmp2 before it knows whether the triple is good, so this rests on the rule that d_tmp0..2 are
// scratch of the call that fills them and hold nothing that outlives it (level-0 results live in d_bh and on the host).
int fw_set_data_csc_f32_resident(fw_ctx *c, const int64_t *colptr, const int32_t *rowval, const float *nzval)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_f32_resident: context is not FW_FZ_NZ");
    if (!c->P.recursive_pcor)
        return fw_fail(c, FW_ERR_LIMIT, "fw_set_data_csc_f32_resident: recursive_pcor = 0 is not served on the CSC-resident layout (its kernels "
                                        "stream whole dense columns); use fw_set_data_csc_f32");
    if (!colptr || (colptr[c->P.p] > 0 && (!rowval || !nzval))) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_f32_resident: NULL array");
    int rc = fwi_fznz_upload_csc_resident(c, colptr, rowval, nzval);  // (a refused triple leaves the context as it was)
    if (rc) return rc;
    c->have_data = true;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_data_resident_bytes(const fw_ctx *c, int64_t *bytes)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_data_resident_bytes: context is not FW_FZ_NZ");
    if (!bytes) return fw_fail(c, FW_ERR_ARG, "fw_data_resident_bytes: NULL output");
    if (!c->have_data) return fw_fail(c, FW_ERR_STATE, "fw_data_resident_bytes: no data uploaded");
    const int64_t cells = (int64_t)c->P.p * c->W;
    // the sizes asked of the allocator: values (matrix, or vals with its one-float minimum), plane, base
    if (c->csc_resident)
        *bytes = 4 * std::max<int64_t>(c->cvals_n, 1) + 8 * cells + 4 * cells;
    else
        *bytes = 4 * (int64_t)c->P.n * c->P.p + 8 * cells;
    return FW_OK;
}

int fw_set_data_dense_i32(fw_ctx *c, const int32_t *data)
{
    CHECK_CTX(c);
    if (c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_i32: context is not discrete");
    if (!data) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_i32: NULL data");
    const int n = c->P.n, p = c->P.p;
    std::vector<int64_t> colptr(p + 1, 0);
    std::vector<int32_t> rowval, nzval;
    for (int v = 0; v < p; ++v) {
        for (int i = 0; i < n; ++i) {
            int32_t x = data[(size_t)v * n + i];
            if (x != 0) {
                rowval.push_back(i);
                nzval.push_back(x);
            }
        }
        colptr[v + 1] = (int64_t)rowval.size();
    }
    return fw_set_data_csc_i32(c, colptr.data(), rowval.data(), nzval.data());
}

// ---- tables that already live in device memory (a torch tensor's data_ptr(), a ROCArray): nothing crosses to the host but the small
// column records of the discrete scan.  The pointer is asked of the runtime before anything reads it; each call synchronises the
// context's stream before it returns.
int fw_set_data_dense_i32_dev(fw_ctx *c, const int32_t *d_data)
{
    CHECK_CTX(c);
    if (c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_i32_dev: context is not discrete");
    if (!d_data) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_i32_dev: NULL data");
    if (!fw_is_dev_ptr(d_data, c->P.device))
        return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_i32_dev: data is not device memory of device %d (fw_set_data_dense_i32 takes a host table)", c->P.device);
    int rc = fwi_mi_upload_dev(c, d_data);
    if (rc) return rc;
    resolve_n_obs_min_discrete(c);
    c->have_data = true;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_set_data_dense_f32_dev(fw_ctx *c, const float *d_data)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ && c->P.kind != FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_f32_dev: context is not FW_FZ / FW_FZ_NZ");
    if (!d_data) return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_f32_dev: NULL data");
    if (!fw_is_dev_ptr(d_data, c->P.device))
        return fw_fail(c, FW_ERR_ARG, "fw_set_data_dense_f32_dev: data is not device memory of device %d (fw_set_data_dense_f32 takes a host matrix)", c->P.device);
    if (c->f64) return fw_fail(c, FW_ERR_STATE, "fw_set_data_dense_f32_dev: the context is in Float64 mode (fw_set_data_dense_f64 / fw_set_cor_mat_f64 came first); precisions do not mix");
    if (c->P.kind == FW_FZ_NZ) {
        int rc = fwi_fznz_upload_dev(c, d_data);
        if (rc) return rc;
        c->have_data = true;
        c->have_level0 = false;
        c->have_network = false;
        return FW_OK;
    }
    const size_t bytes = sizeof(float) * (size_t)c->P.n * c->P.p;
    if (!c->d_data) FW_HIP(c, hipMalloc(&c->d_data, bytes));
    FW_HIP(c, hipMemcpyAsync(c->d_data, d_data, bytes, hipMemcpyDeviceToDevice, c->stream));
    FW_HIP(c, hipStreamSynchronize(c->stream));
    c->f32_input = true;
    c->have_data = true;
    c->have_fzs_stat = false;
    c->have_cor = false;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

// ---- CSC triples that already live in device memory (a sparse torch tensor's three arrays): borrowed where they lie.  Every pointer
// is asked of the runtime, then the p + 1 column pointers are downloaded and checked, before any kernel reads rowval or nzval.  The
// kernels, the state rules and the refusals are those of the host forms.
int fw_set_data_csc_i32_dev(fw_ctx *c, const int64_t *d_colptr, const int32_t *d_rowval, const int32_t *d_nzval, int64_t nnz)
{
    CHECK_CTX(c);
    if (c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_i32_dev: context is not discrete");
    if (int rc = fwi_csc_dev_ptrs(c, "fw_set_data_csc_i32_dev", c->P.device, d_colptr, d_rowval, d_nzval, nnz)) return rc;
    std::vector<int64_t> colptr;
    if (int rc = fwi_csc_dev_colptr(c, "fw_set_data_csc_i32_dev", d_colptr, c->P.p, nnz, colptr)) return rc;
    int rc = fwi_mi_upload_csc_dev(c, d_colptr, d_rowval, d_nzval, nnz);  // (a refused triple leaves the context as it was)
    if (rc) return rc;
    resolve_n_obs_min_discrete(c);
    c->have_data = true;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_set_data_csc_f32_dev(fw_ctx *c, const int64_t *d_colptr, const int32_t *d_rowval, const float *d_nzval, int64_t nnz)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_f32_dev: context is not FW_FZ_NZ");
    if (int rc = fwi_csc_dev_ptrs(c, "fw_set_data_csc_f32_dev", c->P.device, d_colptr, d_rowval, d_nzval, nnz)) return rc;
    std::vector<int64_t> colptr;
    if (int rc = fwi_csc_dev_colptr(c, "fw_set_data_csc_f32_dev", d_colptr, c->P.p, nnz, colptr)) return rc;
    c->have_data = false;  // (a triple refused from here on leaves the resident layout half written, as in fw_set_data_csc_f32)
    c->have_level0 = false;
    c->have_network = false;
    int rc = fwi_fznz_upload_csc_dev(c, d_colptr, d_rowval, d_nzval, nnz);
    if (rc) return rc;
    c->have_data = true;
    return FW_OK;
}

int fw_set_data_csc_f32_resident_dev(fw_ctx *c, const int64_t *d_colptr, const int32_t *d_rowval, const float *d_nzval, int64_t nnz)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ_NZ) return fw_fail(c, FW_ERR_ARG, "fw_set_data_csc_f32_resident_dev: context is not FW_FZ_NZ");
    if (!c->P.recursive_pcor)
        return fw_fail(c, FW_ERR_LIMIT, "fw_set_data_csc_f32_resident_dev: recursive_pcor = 0 is not served on the CSC-resident layout (its kernels "
                                        "stream whole dense columns); use fw_set_data_csc_f32_dev");
    if (int rc = fwi_csc_dev_ptrs(c, "fw_set_data_csc_f32_resident_dev", c->P.device, d_colptr, d_rowval, d_nzval, nnz)) return rc;
    std::vector<int64_t> colptr;
    if (int rc = fwi_csc_dev_colptr(c, "fw_set_data_csc_f32_resident_dev", d_colptr, c->P.p, nnz, colptr)) return rc;
    int rc = fwi_fznz_upload_csc_resident_dev(c, d_colptr, d_rowval, d_nzval, nnz);  // (a refused triple leaves the context as it was)
    if (rc) return rc;
    c->have_data = true;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_get_levels(const fw_ctx *c, int32_t *levels, int32_t *max_vals)
{
    CHECK_CTX(c);
    if (c->levels.empty()) return fw_fail(c, FW_ERR_STATE, "fw_get_levels: no discrete data uploaded");
    if (levels) memcpy(levels, c->levels.data(), sizeof(int32_t) * c->levels.size());
    if (max_vals) memcpy(max_vals, c->max_vals.data(), sizeof(int32_t) * c->max_vals.size());
    return FW_OK;
}

int64_t fw_effective_n_obs_min(const fw_ctx *c) { return c ? c->n_obs_min_eff : -1; }

int fw_set_row_views(fw_ctx *c, int32_t on)
{
    CHECK_CTX(c);
    c->mi_view = on ? 1 : 0;
    return FW_OK;
}

int fw_set_track_rejections(fw_ctx *c, int32_t on)
{
    CHECK_CTX(c);
    c->track_rej = on ? 1 : 0;
    return FW_OK;
}

int fw_rejections_count(const fw_ctx *c, int64_t *n)
{
    CHECK_CTX(c);
    if (!n) return fw_fail(c, FW_ERR_ARG, "fw_rejections_count: NULL output");
    if (!c->have_rej) return fw_fail(c, FW_ERR_STATE, "fw_rejections_count: no fw_learn_network has run with fw_set_track_rejections(1)");
    *n = (int64_t)c->rej.size();
    return FW_OK;
}

int fw_rejections_get(const fw_ctx *c, fw_rejection *out)
{
    CHECK_CTX(c);
    if (!c->have_rej) return fw_fail(c, FW_ERR_STATE, "fw_rejections_get: no fw_learn_network has run with fw_set_track_rejections(1)");
    if (c->rej.empty()) return FW_OK;
    if (!out) return fw_fail(c, FW_ERR_ARG, "fw_rejections_get: NULL output");
    memcpy(out, c->rej.data(), sizeof(fw_rejection) * c->rej.size());
    return FW_OK;
}

// ---- level 0 --------------------------------------------------------------------------------------
// BH (statfuns.jl:326-350) on the p < alpha subset + neighbour lists (tests.jl:372-388).
static int fw_level0_impl(fw_ctx *c, int64_t *nnz_out, int rank, int world, fw_allgather_fn allgather, void *user,
                          const fw_dev_exchange *xdev = nullptr);

int fw_level0(fw_ctx *c, int64_t *nnz_out) { return fw_level0_impl(c, nnz_out, 0, 1, nullptr, nullptr); }

int fw_level0_sharded_dev(fw_ctx *c, int32_t rank, int32_t world_size, const fw_dev_exchange *x, int64_t *nnz_out)
{
    CHECK_CTX(c);
    if (world_size < 1 || rank < 0 || rank >= world_size) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded_dev: rank %d outside world of %d", rank, world_size);
    if (world_size > 1 && (!x || !x->prepare || !x->exchange)) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded_dev: world_size > 1 needs both exchange callbacks");
    if (c->f64) return fw_fail(c, FW_ERR_LIMIT, "fw_level0_sharded_dev is not served in Float64 mode");
    return fw_level0_impl(c, nnz_out, rank, world_size, nullptr, nullptr, x);
}

int fw_use_cor_buffer(fw_ctx *c, void *d_cor, int64_t capacity_floats)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ) return fw_fail(c, FW_ERR_ARG, "fw_use_cor_buffer: context is not FW_FZ");
    if (c->P.no_cor_mat) return fw_fail(c, FW_ERR_STATE, "fw_use_cor_buffer: the context was created with no_cor_mat (dense_cor = false)");
    if (c->f64) return fw_fail(c, FW_ERR_LIMIT, "fw_use_cor_buffer is not served in Float64 mode");
    if (!d_cor || capacity_floats < (int64_t)c->P.p * c->P.p) return fw_fail(c, FW_ERR_ARG, "fw_use_cor_buffer: needs at least p * p floats of device memory");
    if (c->d_cor && !c->cor_external) (void)hipFree(c->d_cor);
    c->d_cor = (float *)d_cor;
    c->cor_external = true;
    c->cor_capacity = capacity_floats;
    c->have_cor = false;
    c->have_level0 = false;
    c->have_network = false;
    return FW_OK;
}

int fw_compute_cor_mat_rows(fw_ctx *c, int32_t rank, int32_t world_size, int64_t *row0, int64_t *rows_per_rank)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ) return fw_fail(c, FW_ERR_ARG, "fw_compute_cor_mat_rows: context is not FW_FZ");
    if (c->P.no_cor_mat) return fw_fail(c, FW_ERR_STATE, "fw_compute_cor_mat_rows: the context was created with no_cor_mat (dense_cor = false)");
    if (world_size < 1 || rank < 0 || rank >= world_size || !row0 || !rows_per_rank) return fw_fail(c, FW_ERR_ARG, "fw_compute_cor_mat_rows: invalid argument");
    if (c->f64) return fw_fail(c, FW_ERR_LIMIT, "fw_compute_cor_mat_rows is not served in Float64 mode");
    c->have_level0 = false;
    c->have_network = false;
    return fwi_fz_compute_cor_rows(c, rank, world_size, row0, rows_per_rank);
}

int fw_cor_mat_ready(fw_ctx *c)
{
    CHECK_CTX(c);
    if (c->P.kind != FW_FZ || !c->d_cor) return fw_fail(c, FW_ERR_STATE, "fw_cor_mat_ready: no correlation matrix buffer");
    c->have_cor = true;
    return FW_OK;
}

int fw_level0_sharded(fw_ctx *c, int32_t rank, int32_t world_size, fw_allgather_fn allgather, void *user, int64_t *nnz_out)
{
    CHECK_CTX(c);
    if (world_size < 1 || rank < 0 || rank >= world_size) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded: rank %d outside world of %d", rank, world_size);
    if (world_size > 1 && !allgather) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded: world_size > 1 needs an allgather callback");
    if (c->f64) return fw_fail(c, FW_ERR_LIMIT, "fw_level0_sharded is not served in Float64 mode");
    return fw_level0_impl(c, nnz_out, rank, world_size, allgather, user);
}

// What one fw_level0 call carries from stage to stage: the significant pairs on the host (host exchange, host epilogue) and / or as
// the kernels left them in device memory, and the number of reliable tests BH divides by.
struct L0Run {
    std::vector<int32_t> pi, pj;
    std::vector<double> stat, pval;
    int64_t m = 0;
    FwL0Dev dev;
};

static int l0_precheck(fw_ctx *c)
{
    if (c->P.kind == FW_FZ && !c->P.no_cor_mat) {
        if (!c->have_cor) {
            int rc = c->f64 ? fwi_fz64_compute_cor(c) : fwi_fz_compute_cor(c);
            if (rc) return rc;
        }
    } else if (!c->have_data) {  // (no_cor_mat: the level-0 kernels multiply and screen the centred columns themselves)
        return fw_fail(c, FW_ERR_STATE, "fw_level0: no data uploaded");
    }
    if (c->n_obs_min_eff > c->P.n)  // learning.jl:66-73
        return fw_fail(c, FW_ERR_NOBS,
                       "Dataset has an insufficient number of observations, need at least %lld ('n_obs_min') for reliable tests",
                       (long long)c->n_obs_min_eff);
    return FW_OK;
}

// The pair screen of the context's kind; a sharded run screens this rank's share of the pair tiles.  want_dev: leave the pairs in
// device memory (r.dev) instead of the host vectors.
static int l0_screen(fw_ctx *c, L0Run &r, int rank, int world, bool want_dev)
{
    FwL0Dev *devp = want_dev ? &r.dev : nullptr;
    c->l0_rank = rank;
    c->l0_world = world;
    int rc = (c->P.kind == FW_FZ)      ? (c->f64 ? fwi_fz64_level0(c, r.pi, r.pj, r.stat, r.pval, &r.m, devp) : fwi_fz_level0(c, r.pi, r.pj, r.stat, r.pval, &r.m, devp))
             : (c->P.kind == FW_FZ_NZ) ? fwi_fznz_level0(c, r.pi, r.pj, r.stat, r.pval, &r.m, devp)
                                       : fwi_mi_level0(c, r.pi, r.pj, r.stat, r.pval, &r.m, devp);
    c->l0_rank = 0;
    c->l0_world = 1;
    return rc;
}

// Sharded exchange through the caller's host all-gather: one extra record carries this rank's count of reliable tests
static int l0_exchange_host(fw_ctx *c, L0Run &r, int rank, int world, fw_allgather_fn allgather, void *user)
{
    r.pi.push_back(-1);
    r.pj.push_back(rank);
    r.stat.push_back((double)r.m);
    r.pval.push_back(0.0);
    int64_t ntot = 0;
    const int32_t *ai = nullptr, *aj = nullptr;
    const double *as = nullptr, *ap = nullptr;
    int rc = allgather(user, (int64_t)r.pi.size(), r.pi.data(), r.pj.data(), r.stat.data(), r.pval.data(), &ntot, &ai, &aj, &as, &ap);
    if (rc) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded: allgather callback failed (%d)", rc);
    L0Run all;
    const int nrec = fw_l0_split_gathered(ntot, ai, aj, as, ap, world, (int64_t)c->P.p * (c->P.p - 1) / 2, all.pi, all.pj, all.stat, all.pval, &all.m);
    if (nrec != world) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded: %d of %d ranks reported", nrec, world);
    r = std::move(all);
    return FW_OK;
}

// Sharded exchange with the payload on the device: pack -> caller's collective -> unpack (fw_xchg.hip), the same rule for m
static int l0_exchange_dev(fw_ctx *c, L0Run &r, int world, const fw_dev_exchange *xdev)
{
    FwL0Dev merged;
    int64_t msum = 0;
    if (int rc = fwi_l0_exchange_dev(c, xdev, world, r.dev, r.m, &merged, &msum)) return rc;
    r.dev = merged;
    r.m = msum - (int64_t)(world - 1) * ((int64_t)c->P.p * (c->P.p - 1) / 2);
    return FW_OK;
}

// The host's merged pairs back to the device (d_tmp1 / d_tmp2) for the device epilogue
static int l0_upload(fw_ctx *c, L0Run &r)
{
    const size_t k = r.pi.size();
    if (int rc = fw_dev_reserve(c, c->d_tmp1, (k + 1) * 2 * sizeof(int32_t))) return rc;
    if (int rc = fw_dev_reserve(c, c->d_tmp2, (k + 1) * 2 * sizeof(double))) return rc;
    int32_t *oi = (int32_t *)c->d_tmp1.ptr, *oj = oi + k;
    double *os = (double *)c->d_tmp2.ptr, *op = os + k;
    if (k) {
        FW_HIP(c, hipMemcpyAsync(oi, r.pi.data(), k * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        FW_HIP(c, hipMemcpyAsync(oj, r.pj.data(), k * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
        FW_HIP(c, hipMemcpyAsync(os, r.stat.data(), k * sizeof(double), hipMemcpyHostToDevice, c->stream));
        FW_HIP(c, hipMemcpyAsync(op, r.pval.data(), k * sizeof(double), hipMemcpyHostToDevice, c->stream));
        FW_HIP(c, hipStreamSynchronize(c->stream));
    }
    r.dev = FwL0Dev{};
    r.dev.i = oi;
    r.dev.j = oj;
    r.dev.stat64 = os;
    r.dev.pval = op;
    r.dev.k = k;
    return FW_OK;
}

// BH + neighbour lists on the device (fw_bh.hip); the time includes its device-to-host copies
static int l0_epilogue_dev(fw_ctx *c, const L0Run &r)
{
    const double t0 = fwi_now_s();
    if (int rc = fwi_bh_csr_device(c, r.dev, r.m)) return rc;
    c->cnt.t_level0_host_s += fwi_now_s() - t0;
    return FW_OK;
}

// FW_HOST_BH=1: the host restatement (fw_level0_host.h); the lists then live on the host only
static void l0_epilogue_host(fw_ctx *c, L0Run &r)
{
    c->d_nb_off = nullptr;
    c->d_nb_idx = nullptr;
    c->d_nb_stat = c->d_nb_p = nullptr;
    c->d_cand = nullptr;
    c->nb_host_valid = true;
    const double t0 = fwi_now_s();
    if (c->P.fdr) fw_bh_adjust(r.pval, r.m);
    fw_nb_csr(c->P.p, r.pi, r.pj, r.stat, r.pval, c->P.alpha, c->nb_off, c->nb_idx, c->nb_stat, c->nb_p);
    c->cnt.t_level0_host_s += fwi_now_s() - t0;
}

static int l0_finish(fw_ctx *c, double t_start, int64_t *nnz_out)
{
    c->have_level0 = true;
    c->have_network = false;
    c->cnt.level0_tests += (int64_t)c->P.p * (c->P.p - 1) / 2;
    c->cnt.t_level0_s += fwi_now_s() - t_start;
    if (nnz_out) *nnz_out = c->nb_off[c->P.p];
    return FW_OK;
}

// Target-sharded runs: for the discrete kinds, whose pair screen is the expensive part of level 0 (cfg4: 73 of
// 140 ms), every rank screens its share of the pair tiles and the significant pairs are all-gathered; the Fisher-z kinds screen a
// resident matrix in well under a millisecond per 10^8 pairs and stay replicated.  BH and the neighbour lists are then built
// redundantly on every rank from the same merged list (their result does not depend on the order of the list).
static int fw_level0_impl(fw_ctx *c, int64_t *nnz_out, int rank, int world, fw_allgather_fn allgather, void *user,
                          const fw_dev_exchange *xdev)
{
    CHECK_CTX(c);
    const double t0 = fwi_now_s();
    if (int rc = l0_precheck(c)) return rc;
    // BH + neighbour lists run on the device (fw_bh.hip); FW_HOST_BH=1 keeps the host restatement, which tests/test_gpu_*.py use to
    // cross-check the two
    const bool host_bh = fw_knob_int(knob::FW_HOST_BH, 0) == 1;
    const bool sharded = world > 1 && (c->P.kind == FW_MI || c->P.kind == FW_MI_NZ);
    const bool via_host = sharded && !xdev;  // the pairs cross the host all-gather: the screen leaves them on the host
    L0Run r;
    if (int rc = l0_screen(c, r, sharded ? rank : 0, sharded ? world : 1, !host_bh && !via_host)) return rc;
    if (sharded && xdev) {
        if (host_bh) return fw_fail(c, FW_ERR_ARG, "fw_level0_sharded_dev: FW_HOST_BH=1 is a single-rank debugging mode");
        if (int rc = l0_exchange_dev(c, r, world, xdev)) return rc;
    } else if (sharded) {
        if (int rc = l0_exchange_host(c, r, rank, world, allgather, user)) return rc;
        if (!host_bh)
            if (int rc = l0_upload(c, r)) return rc;
    }
    if (host_bh)
        l0_epilogue_host(c, r);
    else if (int rc = l0_epilogue_dev(c, r))
        return rc;
    return l0_finish(c, t0, nnz_out);
}

int fw_level0_get(const fw_ctx *c, int64_t *off, int32_t *idx, double *stat, double *adj_p)
{
    CHECK_CTX(c);
    if (!c->have_level0) return fw_fail(c, FW_ERR_STATE, "fw_level0_get: fw_level0 has not run");
    if (int rc = fwi_nb_host_ensure(const_cast<fw_ctx *>(c))) return rc;  // lists may still live on the device only
    if (off) memcpy(off, c->nb_off.data(), sizeof(int64_t) * c->nb_off.size());
    const size_t tot = c->nb_idx.size();
    if (idx && tot) memcpy(idx, c->nb_idx.data(), sizeof(int32_t) * tot);
    if (stat && tot) memcpy(stat, c->nb_stat.data(), sizeof(double) * tot);
    if (adj_p && tot) memcpy(adj_p, c->nb_p.data(), sizeof(double) * tot);
    return FW_OK;
}

// ---- per-pair batches --------------------------------------------------------------------------------
static int check_var(const fw_ctx *c, int32_t v) { return v >= 0 && v < c->P.p; }

int fw_test_batch(fw_ctx *c, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff, const int32_t *zflat,
                  fw_test_result *out)
{
    CHECK_CTX(c);
    if (m < 0 || (m > 0 && (!X || !Y || !zoff || !out))) return fw_fail(c, FW_ERR_ARG, "fw_test_batch: NULL argument");
    if (m == 0) return FW_OK;
    for (int64_t t = 0; t < m; ++t) {
        const int64_t k = zoff[t + 1] - zoff[t];
        if (k < 0 || k > FW_MAX_K) return fw_fail(c, FW_ERR_LIMIT, "fw_test_batch: test %lld has %lld conditioning variables (max %d)", (long long)t, (long long)k, FW_MAX_K);
        if (!check_var(c, X[t]) || !check_var(c, Y[t])) return fw_fail(c, FW_ERR_ARG, "fw_test_batch: variable index out of range in test %lld", (long long)t);
        for (int64_t q = zoff[t]; q < zoff[t + 1]; ++q)
            if (!check_var(c, zflat[q])) return fw_fail(c, FW_ERR_ARG, "fw_test_batch: conditioning variable out of range in test %lld", (long long)t);
    }
    if (c->P.kind == FW_FZ && !c->P.recursive_pcor) {
        // no cor_mat for conditional tests (tests.jl:253 -> pcor): they stream their sample columns; univariate tests keep
        // the matrix path (level 0 computes the matrix anyway)
        if (!c->have_data) return fw_fail(c, FW_ERR_STATE, "fw_test_batch: no data uploaded");
        if ((int64_t)c->P.n < c->n_obs_min_eff) {
            fw_fill_no_power(out, m);
            return FW_OK;
        }
        std::vector<int64_t> iu, ic;
        // (no_cor_mat: univariate tests come from the data too -- Float64 sums of the two columns, not the Float32 MFMA value level 0 screens)
        for (int64_t t = 0; t < m; ++t) ((zoff[t + 1] == zoff[t] && !c->P.no_cor_mat) ? iu : ic).push_back(t);
        for (int part = 0; part < 2; ++part) {
            const std::vector<int64_t> &ix = part ? ic : iu;
            if (ix.empty()) continue;
            if (part == 0 && !c->have_cor)
                if (int rc = fwi_fz_compute_cor(c)) return rc;
            std::vector<int32_t> x2(ix.size()), y2(ix.size()), zf;
            std::vector<int64_t> zo(ix.size() + 1, 0);
            for (size_t q = 0; q < ix.size(); ++q) {
                x2[q] = X[ix[q]];
                y2[q] = Y[ix[q]];
                zf.insert(zf.end(), zflat + zoff[ix[q]], zflat + zoff[ix[q] + 1]);
                zo[q + 1] = (int64_t)zf.size();
            }
            if (zf.empty()) zf.push_back(0);
            std::vector<fw_test_result> o2(ix.size());
            const int rc = part ? fwi_fzs_test_batch(c, (int64_t)ix.size(), x2.data(), y2.data(), zo.data(), zf.data(), o2.data())
                                : fwi_fz_test_batch(c, (int64_t)ix.size(), x2.data(), y2.data(), zo.data(), zf.data(), o2.data());
            if (rc) return rc;
            for (size_t q = 0; q < ix.size(); ++q) out[ix[q]] = o2[q];
        }
        return FW_OK;
    }
    if (c->P.kind == FW_FZ) {
        if (!c->have_cor) return fw_fail(c, FW_ERR_STATE, "fw_test_batch: no correlation matrix (fw_compute_cor_mat / fw_set_cor_mat)");
        if (c->f64) {
            for (int64_t t = 0; t < m; ++t)
                if (zoff[t + 1] - zoff[t] > FW_MAX_K_FAST)
                    return fw_fail(c, FW_ERR_LIMIT, "fw_test_batch: test %lld has %lld conditioning variables; Float64 mode serves up to %d", (long long)t,
                                   (long long)(zoff[t + 1] - zoff[t]), FW_MAX_K_FAST);
            return fwi_fz64_test_batch(c, m, X, Y, zoff, zflat, out);
        }
        return fwi_fz_test_batch(c, m, X, Y, zoff, zflat, out);
    }
    if (!c->have_data) return fw_fail(c, FW_ERR_STATE, "fw_test_batch: no data uploaded");
    if (c->P.kind == FW_FZ_NZ) {
        if ((int64_t)c->P.n < c->n_obs_min_eff) {  // tests.jl:11 / :254 on the full row count
            fw_fill_no_power(out, m);
            return FW_OK;
        }
        return fwi_fznz_test_batch(c, m, X, Y, zoff, zflat, out);
    }
    return fwi_mi_test_batch(c, m, X, Y, zoff, zflat, out);
}

}  // extern "C"

static double binom_d(int n, int k)
{
    if (k < 0 || k > n) return 0.0;
    double r = 1.0;
    for (int i = 1; i <= k; ++i) r = r * (double)(n - k + i) / (double)i;
    return std::floor(r + 0.5);
}

double fwi_alg_bytes(const fw_ctx *c, int a, int64_t evaluated)
{
    double bytes = 0.0, left = (double)evaluated;
    for (int s = c->P.max_k; s >= 1 && left > 0; --s) {
        const double cnt = std::min(left, binom_d(a, s));
        double per;
        if (c->P.kind == FW_FZ && !c->P.recursive_pcor)  // streaming variant: k + 2 sample columns per test (B_fzS)
            per = (double)(s + 2) * (double)c->P.n * 4.0 + 32.0;
        else if (c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ)  // gather variant (fz_nz: on the job-local matrix)
            per = 4.0 * (double)((s + 2) * (s + 1) / 2) + 32.0;
        else
            per = (double)(s + 2) * (double)c->P.n * (c->P.kind == FW_MI ? 1.0 : 2.0) / 8.0 + 32.0;
        bytes += cnt * per;
        left -= cnt;
    }
    return bytes;
}

extern "C" {

int fw_test_subsets_batch(fw_ctx *c, int64_t m, const int32_t *T, const int32_t *cand, const int64_t *accoff,
                          const int32_t *accflat, fw_subsets_result *out)
{
    CHECK_CTX(c);
    if (m < 0 || (m > 0 && (!T || !cand || !accoff || !out))) return fw_fail(c, FW_ERR_ARG, "fw_test_subsets_batch: NULL argument");
    if (m == 0) return FW_OK;
    // FW_FZ with the recursive form reads the resident Pearson matrix; with recursive_pcor = 0 the tests stream the sample columns
    // and need the data only (the same split as fw_test_batch)
    const bool needs_cor = c->P.kind == FW_FZ && c->P.recursive_pcor;
    if (needs_cor ? !c->have_cor : !c->have_data)
        return fw_fail(c, FW_ERR_STATE, "fw_test_subsets_batch: no %s resident", needs_cor ? "correlation matrix" : "data");
    if (c->P.max_k < 1) return fw_fail(c, FW_ERR_ARG, "fw_test_subsets_batch: max_k must be >= 1");
    std::vector<FwJob> jobs;
    std::vector<int64_t> map;
    jobs.reserve((size_t)m);
    for (int64_t i = 0; i < m; ++i) {
        const int64_t len = accoff[i + 1] - accoff[i];
        if (len < 0 || len > INT32_MAX) return fw_fail(c, FW_ERR_ARG, "fw_test_subsets_batch: bad accoff at job %lld", (long long)i);
        if (!check_var(c, T[i]) || !check_var(c, cand[i])) return fw_fail(c, FW_ERR_ARG, "fw_test_subsets_batch: variable out of range in job %lld", (long long)i);
        for (int64_t q = accoff[i]; q < accoff[i + 1]; ++q)
            if (!check_var(c, accflat[q])) return fw_fail(c, FW_ERR_ARG, "fw_test_subsets_batch: accepted variable out of range in job %lld", (long long)i);
        if (len == 0) {  // tests.jl:285 sentinel
            fw_subsets_result r{};
            r.stat = NAN;
            r.pval = NAN;
            r.df = -1;
            r.suff_power = 1;
            r.status = FW_SUBSETS_EMPTY;
            r.n_zs = 0;
            r.num_tests = -1;
            r.frac = NAN;
            out[i] = r;
            continue;
        }
        FwJob j{};
        j.X = T[i];
        j.Y = cand[i];
        j.acc_off = accoff[i];
        j.acc_len = (int32_t)len;
        jobs.push_back(j);
        map.push_back(i);
    }
    std::vector<FwJobOut> jo(jobs.size());
    int rc = fwi_subsets_dispatch(c, (int64_t)jobs.size(), jobs.data(), accflat, accoff[m], jo.data());
    if (rc) return rc;
    for (size_t q = 0; q < jobs.size(); ++q) {
        const FwJobOut &o = jo[q];
        fw_subsets_result r{};
        r.stat = o.stat;
        r.pval = o.pval;
        r.df = o.df;
        r.suff_power = o.suff_power;
        r.status = o.status;
        r.n_zs = o.n_zs;
        for (int z = 0; z < FW_MAX_K; ++z) r.zs[z] = z < o.n_zs ? o.zs[z] : 0;
        r.num_tests = o.num_tests;
        double total = 0.0;  // tests.jl:313,327-332
        for (int s = c->P.max_k; s >= 1; --s) total += binom_d(jobs[q].acc_len, s);
        r.frac = total > 0 ? (double)o.num_tests / total : NAN;
        out[map[q]] = r;
        c->cnt.cond_tests_ref += o.num_tests;
        c->cnt.cond_tests_evaluated += o.evaluated;
        c->cnt.alg_bytes_subsets += fwi_alg_bytes(c, jobs[q].acc_len, o.evaluated);
        c->cnt.subsets_calls += 1;
    }
    return FW_OK;
}

int fw_get_counters(const fw_ctx *c, fw_counters *out)
{
    CHECK_CTX(c);
    if (!out) return fw_fail(c, FW_ERR_ARG, "fw_get_counters: NULL output");
    *out = c->cnt;
    return FW_OK;
}

int fw_selftest(fw_ctx *c, int which, uint64_t cases, uint64_t seed, uint64_t *mismatches)
{
    if (!c || !mismatches) return fw_fail(c, FW_ERR_ARG, "fw_selftest: NULL argument");
    *mismatches = 0;
    if (which == FW_SELFTEST_DIV) {
        unsigned long long bad = 0;
        const int rc = fwi_selftest_div(c, (unsigned long long)cases, (unsigned long long)seed, &bad);
        *mismatches = (uint64_t)bad;
        return rc;
    }
    return fw_fail(c, FW_ERR_ARG, "fw_selftest: unknown test %d", which);
}

int fw_reset_counters(fw_ctx *c)
{
    CHECK_CTX(c);
    c->cnt = fw_counters{};
    return FW_OK;
}

}  // extern "C"
