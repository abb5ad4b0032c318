// FlashWeave-S (Fisher-z) in Float64 for gfx950: learn_network(prec = 64).  The whole continuous pipeline of the reference takes its
// element type from `prec` (learning.jl:42-45: cor_mat = convert(Matrix{cont_type}, cor(data_dense)); pcor_rec rounds in that type,
// statfuns.jl:23-75); a context enters this mode through fw_set_data_dense_f64 / fw_set_cor_mat_f64 and then keeps a p x p Float64
// matrix resident next to nothing of the Float32 path.
//
//   Pearson matrix     centring in Float64, Gram product on v_mfma_f64_16x16x4_f64, cov2cor epilogue with mirrored writes
//   level 0            |r| screen against the thresholds of fz_thresholds_kernel, exact p-value for the pairs that pass
//   single tests       one lane per test: fw_pcor64 (fw_pcor64.h) + the p-value of the Float32 path (fz_pval_slow)
//   test_subsets       the general form (fz_subsets_slow_kernel's shape): one workgroup per FwSeg, a run of consecutive ranks per thread
//   HITON-PC           host job pool only (fw_hiton.cpp: choose_path), over the segment kernel here
//
// No table / threshold / device-round kernels: those of fw_fz_core.h and fw_devhiton.hip are tuned around 4-byte entries.
// Compiled with -ffp-contract=off (fw_pcor64.h depends on it).
#include "fw_internal.h"
#include "fw_pcor64.h"
#include "fw_fz_core.h"  // fz_pval_slow: the same log / erfc sequence as the Float32 path

#include <algorithm>
#include <cmath>

// ------------------------------------------------------------------------------------------------
// 1. centring + column norms, all in Float64.  xc is [p_pad][n_pad], zero padded.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fz64_center_kernel(const double *__restrict__ data, double *__restrict__ xc, double *__restrict__ sd,
                                                          int n, int p, int n_pad)
{
    const int v = blockIdx.x;
    double *dst = xc + (size_t)v * n_pad;
    __shared__ double s_red[4];
    if (v >= p) {
        for (int i = threadIdx.x; i < n_pad; i += 256) dst[i] = 0.0;
        if (threadIdx.x == 0) sd[v] = 0.0;
        return;
    }
    const double *src = data + (size_t)v * n;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += src[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
    __syncthreads();
    const double mean = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (double)n;
    __syncthreads();
    double ss = 0.0;
    for (int i = threadIdx.x; i < n_pad; i += 256) {
        double d = 0.0;
        if (i < n) {
            d = src[i] - mean;
            ss += d * d;
        }
        dst[i] = d;
    }
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = ss;
    __syncthreads();
    if (threadIdx.x == 0) sd[v] = sqrt(s_red[0] + s_red[1] + s_red[2] + s_red[3]);
}

// ------------------------------------------------------------------------------------------------
// 2. C = Xc' Xc on v_mfma_f64_16x16x4_f64, 128 x 128 tiles of the upper triangle, cov2cor epilogue.
//    Operands: lane l holds A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15], one Float64 each.
//    C/D (NOT the map of the other MFMA shapes): register r of lane l is C[row (l >> 4) + 4 r][col l & 15].
//    Four wavefronts, 64 x 64 each = 4 x 4 MFMA tiles (64 accumulator doubles per lane); per k-tile of 16 samples a wavefront reads
//    8 doubles per lane and k-step from LDS for 16 MFMAs.  LDS rows are 18 doubles: 16-byte aligned for the b128 stores, and the 16
//    rows x 2 k of a half-wave's b64 reads fall on 32 different 8-byte banks.
//    The next k-tile is fetched into registers before the MFMA block of the current one.
// ------------------------------------------------------------------------------------------------
typedef double f64x4 __attribute__((ext_vector_type(4)));
#define G64_BM 128
#define G64_BK 16
#define G64_LD (G64_BK + 2)

__global__ __launch_bounds__(256) void fz64_gram_kernel(const double *__restrict__ xc, const double *__restrict__ sd, double *__restrict__ cor,
                                                        int p, int n_pad)
{
    __shared__ __attribute__((aligned(16))) double sA[G64_BM * G64_LD];
    __shared__ __attribute__((aligned(16))) double sB[G64_BM * G64_LD];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;  // upper triangle; the mirror image is written by the tile that computes (bi, bj)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lr = lane & 15, lk = lane >> 4;
    // global -> LDS staging: 128 columns x 16 k = 1024 double2 per operand, 4 per thread; 8 consecutive lanes cover one 128-byte row
    const int ld_col = tid >> 3, ld_k2 = tid & 7;
    const double *pA = xc + ((size_t)bi * G64_BM + ld_col) * n_pad + ld_k2 * 2;
    const double *pB = xc + ((size_t)bj * G64_BM + ld_col) * n_pad + ld_k2 * 2;
    const size_t cstep = (size_t)32 * n_pad;

    f64x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f64x4){0.0, 0.0, 0.0, 0.0};

    double2 ra0, ra1, ra2, ra3, rb0, rb1, rb2, rb3;
#define G64_GLOAD(k0)                                                   \
    do {                                                                \
        ra0 = *reinterpret_cast<const double2 *>(pA + (k0));            \
        ra1 = *reinterpret_cast<const double2 *>(pA + cstep + (k0));    \
        ra2 = *reinterpret_cast<const double2 *>(pA + 2 * cstep + (k0)); \
        ra3 = *reinterpret_cast<const double2 *>(pA + 3 * cstep + (k0)); \
        rb0 = *reinterpret_cast<const double2 *>(pB + (k0));            \
        rb1 = *reinterpret_cast<const double2 *>(pB + cstep + (k0));    \
        rb2 = *reinterpret_cast<const double2 *>(pB + 2 * cstep + (k0)); \
        rb3 = *reinterpret_cast<const double2 *>(pB + 3 * cstep + (k0)); \
    } while (0)
    G64_GLOAD(0);
    for (int k0 = 0; k0 < n_pad; k0 += G64_BK) {
        __syncthreads();  // the previous tile has been read by every wavefront
        {
            double *wa = &sA[ld_col * G64_LD + ld_k2 * 2], *wb = &sB[ld_col * G64_LD + ld_k2 * 2];
            *reinterpret_cast<double2 *>(wa) = ra0;
            *reinterpret_cast<double2 *>(wa + 32 * G64_LD) = ra1;
            *reinterpret_cast<double2 *>(wa + 64 * G64_LD) = ra2;
            *reinterpret_cast<double2 *>(wa + 96 * G64_LD) = ra3;
            *reinterpret_cast<double2 *>(wb) = rb0;
            *reinterpret_cast<double2 *>(wb + 32 * G64_LD) = rb1;
            *reinterpret_cast<double2 *>(wb + 64 * G64_LD) = rb2;
            *reinterpret_cast<double2 *>(wb + 96 * G64_LD) = rb3;
        }
        __syncthreads();
        if (k0 + G64_BK < n_pad) G64_GLOAD(k0 + G64_BK);
        const double *cA = &sA[(wm * 64 + lr) * G64_LD + lk], *cB = &sB[(wn * 64 + lr) * G64_LD + lk];
#pragma unroll
        for (int kk = 0; kk < G64_BK; kk += 4) {
            double a[4], b[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                a[t] = cA[t * 16 * G64_LD + kk];
                b[t] = cB[t * 16 * G64_LD + kk];
            }
#pragma unroll
            for (int tm = 0; tm < 4; ++tm)
#pragma unroll
                for (int tn = 0; tn < 4; ++tn) acc[tm][tn] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
        }
    }
#undef G64_GLOAD
    // epilogue: cov2cor! (C[i,j] / (xsd[i] * xsd[j]), clampcor, unit diagonal); (i, j) and its mirror image get the same value.
    // A zero-variance column gives 0 / 0 = NaN for its row and column (the clamps keep a NaN), 1 on the diagonal.
#pragma unroll
    for (int tn = 0; tn < 4; ++tn) {
        const int j = bj * G64_BM + wn * 64 + tn * 16 + lr;
        const double sdj = (j < p) ? sd[j] : 0.0;
#pragma unroll
        for (int tm = 0; tm < 4; ++tm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = bi * G64_BM + wm * 64 + tm * 16 + lk + 4 * r;
                if (i >= p || j >= p) continue;
                double v = acc[tm][tn][r] / (sd[i] * sdj);
                v = v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v);
                if (i == j) v = 1.0;
                cor[(size_t)i * p + j] = v;
                if (bi != bj) cor[(size_t)j * p + i] = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------
// 3. level 0: all pairs i < j of the resident matrix (tests.jl:149-159 + the NaN / m rule of :397-398,522-526).
//    One kernel: |r| below the lower edge of the guard band of fz_thresholds_kernel cannot be significant; every other pair gets
//    its exact p-value here and is kept if p < alpha.  8 x 1024 pairs per workgroup, kept pairs queued in LDS and appended with
//    one atomic per workgroup (fz_level0_kernel's scheme).
// ------------------------------------------------------------------------------------------------
struct Fz64L0Counters {
    unsigned long long n_sig;
    unsigned long long n_nan;
};
#define FZ64_L0_ROWS 8
#define FZ64_L0_COLS 1024
#define FZ64_L0_QCAP 1536
__global__ __launch_bounds__(256) void fz64_level0_kernel(const double *__restrict__ cor, int p, const double *__restrict__ thr, double alpha,
                                                          double zscale, Fz64L0Counters *cnt, unsigned long long cap, int32_t *out_i,
                                                          int32_t *out_j, double *out_r, double *out_p)
{
    __shared__ int s_qi[FZ64_L0_QCAP], s_qj[FZ64_L0_QCAP];
    __shared__ double s_qr[FZ64_L0_QCAP], s_qp[FZ64_L0_QCAP];
    __shared__ int s_qn;
    __shared__ unsigned long long s_qbase;
    const int i0 = blockIdx.y * FZ64_L0_ROWS;
    const int jb = blockIdx.x * FZ64_L0_COLS;
    if (jb + FZ64_L0_COLS - 1 <= i0) return;  // tile entirely on / below the diagonal
    if (threadIdx.x == 0) s_qn = 0;
    __syncthreads();
    const double lo_pos = thr[0], lo_neg = thr[2];
    unsigned int n_nan = 0;
    for (int ii = 0; ii < FZ64_L0_ROWS; ++ii) {
        const int i = i0 + ii;
        if (i >= p) break;
        const double *row = cor + (size_t)i * p;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int j = jb + u * 256 + threadIdx.x;  // consecutive lanes read consecutive doubles
            if (j <= i || j >= p) continue;
            const double r = row[j];
            if (isnan(r)) {
                ++n_nan;
                continue;
            }
            if (!(fabs(r) >= (r < 0.0 ? lo_neg : lo_pos))) continue;
            const double pv = fz_pval_slow(r, zscale);
            if (!(pv < alpha)) continue;
            const int q = atomicAdd(&s_qn, 1);  // LDS
            if (q < FZ64_L0_QCAP) {
                s_qi[q] = i;
                s_qj[q] = j;
                s_qr[q] = r;
                s_qp[q] = pv;
            } else {
                const unsigned long long slot = atomicAdd(&cnt->n_sig, 1ull);
                if (slot < cap) {
                    out_i[slot] = i;
                    out_j[slot] = j;
                    out_r[slot] = r;
                    out_p[slot] = pv;
                }
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n_nan += __shfl_xor(n_nan, o);
    if ((threadIdx.x & 63) == 0 && n_nan) atomicAdd(&cnt->n_nan, (unsigned long long)n_nan);
    __syncthreads();
    const int nq = s_qn < FZ64_L0_QCAP ? s_qn : FZ64_L0_QCAP;
    if (threadIdx.x == 0 && nq > 0) s_qbase = atomicAdd(&cnt->n_sig, (unsigned long long)nq);
    __syncthreads();
    for (int q = threadIdx.x; q < nq; q += 256) {
        const unsigned long long slot = s_qbase + (unsigned long long)q;
        if (slot < cap) {
            out_i[slot] = s_qi[q];
            out_j[slot] = s_qj[q];
            out_r[slot] = s_qr[q];
            out_p[slot] = s_qp[q];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// 4. batch of single tests (tests.jl:108-160 / 250-265), one lane per test
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void fz64_test_batch_kernel(const double *__restrict__ cor, int p, long long m, const int32_t *__restrict__ X,
                                                              const int32_t *__restrict__ Y, const long long *__restrict__ zoff,
                                                              const int32_t *__restrict__ zflat, double zscale, fw_test_result *__restrict__ out)
{
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= m) return;
    const int k = (int)(zoff[t + 1] - zoff[t]);
    int z[FW_PCOR64_MAX_K];
    for (int q = 0; q < FW_PCOR64_MAX_K; ++q) z[q] = (q < k) ? zflat[zoff[t] + q] : 0;
    const double r = k == 0 ? cor[(size_t)Y[t] * p + X[t]] : fw_pcor64(cor, p, X[t], Y[t], z, k);
    fw_test_result o;
    o.stat = r;
    o.pval = fz_pval_slow(r, zscale);
    o.df = 0;
    o.suff_power = 1;
    out[t] = o;
}

// ------------------------------------------------------------------------------------------------
// 5. test_subsets, general form (the shape of fz_subsets_slow_kernel): one workgroup per segment, every thread a run of
//    consecutive ranks in the reference's order (sizes max_k..1, lexicographic over positions: unranked once, then stepped), every
//    test fw_pcor64 and its exact p-value.  The first non-significant rank or the max_tests stop ends the job; otherwise the `>=`
//    maximum of the p-values with the later rank winning ties (tests.jl:326-341), reduced through LDS.  Writes the FwSegOut record
//    the other segment kernels write: the host merge, the rejection log and the counters are shared.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long fz64_binom_sat(int m, int t)  // C(m, t), t <= 5, saturating at 2^62
{
    if (t < 0 || m < t) return 0ull;
    double est = 1.0;
    for (int i = 1; i <= t; ++i) est = est * (double)(m - t + i) / (double)i;
    if (est > 2.0e18) return 1ull << 62;
    unsigned long long v = 1ull;
    for (int i = 1; i <= t; ++i) v = v * (unsigned long long)(m - t + i) / (unsigned long long)i;
    return v;
}

__global__ __launch_bounds__(256) void fz64_subsets_kernel(const double *__restrict__ cor, int p, const FwSeg *__restrict__ segs,
                                                           const int32_t *__restrict__ accflat, FwSegOut *__restrict__ out, int max_k,
                                                           double alpha, double zscale, long long max_tests)
{
    constexpr int KM = FW_PCOR64_MAX_K;
    __shared__ unsigned long long s_stop[256], s_br[256];
    __shared__ double s_bp[256];
    __shared__ unsigned int s_done[256];
    const FwSeg seg = segs[blockIdx.x];
    FwSegOut *out_rec = out + blockIdx.x;
    const int tid = threadIdx.x, a = seg.acc_len;
    const int32_t *gacc = accflat + seg.acc_off;
    const int X = seg.X, Y = seg.Y;
    unsigned long long cnt[KM + 1];
    for (int s = KM; s >= 1; --s) cnt[s] = (s <= max_k) ? fz64_binom_sat(a, s) : 0ull;
    const unsigned long long len = seg.end - seg.start, R = (len + 255ull) / 256ull;
    const unsigned long long r0 = seg.start + (unsigned long long)tid * R;
    unsigned long long r1 = r0 + R;
    if (r1 > seg.end) r1 = seg.end;
    unsigned long long my_stop = FW_RANK_NONE, my_br = 0ull;
    double stop_stat = 0.0, stop_p = 0.0, my_bp = -1.0, my_bstat = 0.0;
    unsigned int my_done = 0u;
    if (r0 < seg.end) {
        unsigned long long rem = r0;
        int s = max_k < KM ? max_k : KM;
        while (s > 1 && rem >= cnt[s]) {
            rem -= cnt[s];
            --s;
        }
        int pos[KM];
        for (int q = 0; q < KM; ++q) pos[q] = 0;
        {   // position d = the first c whose block of C(a - 1 - c, s - d - 1) subsets holds the rank
            int prev = -1;
            for (int d = 0; d < s; ++d) {
                int c = prev + 1;
                for (;;) {
                    const unsigned long long with_c = fz64_binom_sat(a - 1 - c, s - d - 1);
                    if (rem < with_c || c >= a - 1) break;  // (c >= a - 1: ranks past the enumeration never index beyond the list)
                    rem -= with_c;
                    ++c;
                }
                pos[d] = c;
                prev = c;
            }
        }
        for (unsigned long long r = r0; r < r1; ++r) {
            int zs[KM];
            for (int q = 0; q < KM; ++q) {
                const int ps = pos[q] < a ? pos[q] : a - 1;  // always inside the accepted list
                zs[q] = (q < s) ? gacc[ps] : 0;
            }
            const double stat = fw_pcor64(cor, p, X, Y, zs, s);
            const double pv = fz_pval_slow(stat, zscale);
            ++my_done;
            if (!(pv < alpha) || (max_tests > 0 && r + 1ull >= (unsigned long long)max_tests)) {
                my_stop = r;
                stop_stat = stat;
                stop_p = pv;
                break;
            }
            if (pv >= my_bp) {  // tests.jl:338 `>=`: the later rank wins ties
                my_bp = pv;
                my_bstat = stat;
                my_br = r;
            }
            int i = s - 1;
            while (i >= 0 && pos[i] == a - s + i) --i;
            if (i < 0) {
                --s;
                for (int q = 0; q < KM; ++q) pos[q] = q;
                if (s < 1) break;
            } else {
                ++pos[i];
                for (int j = i + 1; j < s; ++j) pos[j] = pos[j - 1] + 1;
            }
        }
    }
    s_stop[tid] = my_stop;
    s_bp[tid] = my_bp;
    s_br[tid] = my_br;
    s_done[tid] = my_done;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            if (s_stop[tid + o] < s_stop[tid]) s_stop[tid] = s_stop[tid + o];
            if (s_bp[tid + o] > s_bp[tid] || (s_bp[tid + o] == s_bp[tid] && s_br[tid + o] > s_br[tid])) {
                s_bp[tid] = s_bp[tid + o];
                s_br[tid] = s_br[tid + o];
            }
            s_done[tid] += s_done[tid + o];
        }
        __syncthreads();
    }
    const unsigned long long first = s_stop[0];
    FwSegOut o;
    o.stop_df = 0;
    o.best_df = 0;
    o.pad = 0;
    o.evaluated = s_done[0];
    if (first != FW_RANK_NONE) {
        if (my_stop != first) return;
        o.stop_rank = first;
        o.stop_stat = stop_stat;
        o.stop_pval = stop_p;
        o.best_rank = 0;
        o.best_stat = 0.0;
        o.best_pval = -1.0;
        o.stop_power = 1;
        *out_rec = o;
        return;
    }
    if (s_bp[0] < 0.0 ? tid != 0 : !(my_bp == s_bp[0] && my_br == s_br[0] && my_done > 0u)) return;  // the owner of the maximum writes (no test at all: thread 0)
    o.stop_rank = FW_RANK_NONE;
    o.stop_stat = 0.0;
    o.stop_pval = 0.0;
    o.best_rank = s_bp[0] < 0.0 ? 0ull : my_br;
    o.best_stat = s_bp[0] < 0.0 ? 0.0 : my_bstat;
    o.best_pval = s_bp[0] < 0.0 ? -1.0 : my_bp;
    o.stop_power = 1;
    *out_rec = o;
}

// ------------------------------------------------------------------------------------------------
// host launchers
// ------------------------------------------------------------------------------------------------
static double fz64_zscale(const fw_ctx *ctx)
{
    const long long sf = (long long)ctx->P.n - 3;  // len_z = 0 always (tests.jl:156,256)
    return sf > 0 ? std::sqrt((double)sf) / 2.0 : 0.0;
}

// device memory of the Float64 mode: a failed allocation is a capacity answer (FW_ERR_NOMEM), not a device error
static int fz64_alloc(fw_ctx *ctx, double **ptr, size_t doubles, const char *what)
{
    if (*ptr) return FW_OK;
    const hipError_t e = hipMalloc((void **)ptr, doubles * sizeof(double));
    if (e == hipSuccess) return FW_OK;
    *ptr = nullptr;
    (void)hipGetLastError();
    if (e == hipErrorOutOfMemory)
        return fw_fail(ctx, FW_ERR_NOMEM, "Float64 mode: %s needs %.1f MB of device memory (the p x p matrix alone: 8 p^2 bytes)", what,
                       (double)doubles * 8.0 / 1048576.0);
    return fw_fail(ctx, FW_ERR_DEVICE, "hipMalloc (%s) failed: %s", what, hipGetErrorString(e));
}

int fwi_fz64_set_data(fw_ctx *ctx, const double *data)
{
    const size_t cells = (size_t)ctx->P.n * ctx->P.p;
    if (int rc = fz64_alloc(ctx, &ctx->d_data64, cells, "the n x p data")) return rc;
    FW_HIP(ctx, hipMemcpy(ctx->d_data64, data, cells * sizeof(double), hipMemcpyHostToDevice));
    return FW_OK;
}

int fwi_fz64_set_cor(fw_ctx *ctx, const double *cor)
{
    const size_t cells = (size_t)ctx->P.p * ctx->P.p;
    if (int rc = fz64_alloc(ctx, &ctx->d_cor64, cells, "the p x p correlation matrix")) return rc;
    FW_HIP(ctx, hipMemcpy(ctx->d_cor64, cor, cells * sizeof(double), hipMemcpyHostToDevice));
    return FW_OK;
}

int fwi_fz64_get_cor(const fw_ctx *ctx, double *out)
{
    FW_HIP(ctx, hipMemcpy(out, ctx->d_cor64, sizeof(double) * (size_t)ctx->P.p * ctx->P.p, hipMemcpyDeviceToHost));
    return FW_OK;
}

int fwi_fz64_compute_cor(fw_ctx *ctx)
{
    if (!ctx->have_data) return fw_fail(ctx, FW_ERR_STATE, "fw_compute_cor_mat: no data uploaded (fw_set_data_dense_f64)");
    const int n = ctx->P.n, p = ctx->P.p;
    ctx->n_pad = (n + G64_BK - 1) / G64_BK * G64_BK;
    ctx->p_pad = (p + G64_BM - 1) / G64_BM * G64_BM;
    int rc;
    if ((rc = fz64_alloc(ctx, &ctx->d_xc64, (size_t)ctx->n_pad * ctx->p_pad, "the centred columns"))) return rc;
    if ((rc = fz64_alloc(ctx, &ctx->d_sd64, (size_t)ctx->p_pad, "the column norms"))) return rc;
    if ((rc = fz64_alloc(ctx, &ctx->d_cor64, (size_t)p * p, "the p x p correlation matrix"))) return rc;
    hipLaunchKernelGGL(fz64_center_kernel, dim3(ctx->p_pad), dim3(256), 0, ctx->stream, (const double *)ctx->d_data64, ctx->d_xc64, ctx->d_sd64, n,
                       p, ctx->n_pad);
    const int T = ctx->p_pad / G64_BM;
    hipLaunchKernelGGL(fz64_gram_kernel, dim3(T, T), dim3(256), 0, ctx->stream, (const double *)ctx->d_xc64, (const double *)ctx->d_sd64,
                       ctx->d_cor64, p, ctx->n_pad);
    FW_HIP(ctx, hipGetLastError());
    FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->cnt.kernel_launches += 2;
    ctx->have_cor = true;
    return FW_OK;
}

int fwi_fz64_level0(fw_ctx *ctx, std::vector<int32_t> &pi, std::vector<int32_t> &pj, std::vector<double> &stat, std::vector<double> &pval,
                    int64_t *m_reliable, FwL0Dev *dev)
{
    const int p = ctx->P.p;
    const long long npairs = (long long)p * (p - 1) / 2;
    if (ctx->P.n < ctx->n_obs_min_eff) {  // tests.jl:11 -> every test lacks power -> all NaN
        *m_reliable = 0;
        return fwi_l0_handover(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, 0, pi, pj, stat, pval, dev);
    }
    double zscale = 0.0;
    if (int rc = fwi_fz_thresholds(ctx, ctx->stream, &zscale)) return rc;
    Fz64L0Counters h{};
    int32_t *oi = nullptr, *oj = nullptr;
    double *os = nullptr, *op = nullptr;
    const int rc = fwi_l0_attempts(ctx, npairs, 4ll << 20, "Float64 fz level-0: compaction buffer", [&](unsigned long long cap, FwL0Counts &n) -> int {
        int rc;
        if ((rc = fw_dev_reserve(ctx, ctx->d_tmp0, sizeof(Fz64L0Counters)))) return rc;
        if ((rc = fw_dev_reserve(ctx, ctx->d_tmp1, cap * 2 * sizeof(int32_t)))) return rc;
        if ((rc = fw_dev_reserve(ctx, ctx->d_tmp2, cap * 2 * sizeof(double)))) return rc;
        FW_HIP(ctx, hipMemsetAsync(ctx->d_tmp0.ptr, 0, sizeof(Fz64L0Counters), ctx->stream));
        oi = (int32_t *)ctx->d_tmp1.ptr, oj = oi + cap;
        os = (double *)ctx->d_tmp2.ptr, op = os + cap;
        dim3 grid((p + FZ64_L0_COLS - 1) / FZ64_L0_COLS, (p + FZ64_L0_ROWS - 1) / FZ64_L0_ROWS);
        hipLaunchKernelGGL(fz64_level0_kernel, grid, dim3(256), 0, ctx->stream, (const double *)ctx->d_cor64, p, (const double *)ctx->d_thr,
                           ctx->P.alpha, zscale, (Fz64L0Counters *)ctx->d_tmp0.ptr, cap, oi, oj, os, op);
        FW_HIP(ctx, hipGetLastError());
        FW_HIP(ctx, hipMemcpyAsync(&h, ctx->d_tmp0.ptr, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
        FW_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->cnt.kernel_launches += 1;
        n.first = h.n_sig;
        return FW_OK;
    });
    if (rc) return rc;
    *m_reliable = npairs - (long long)h.n_nan;
    return fwi_l0_handover(ctx, oi, oj, os, nullptr, op, (size_t)h.n_sig, pi, pj, stat, pval, dev);
}

int fwi_fz64_test_batch(fw_ctx *ctx, int64_t m, const int32_t *X, const int32_t *Y, const int64_t *zoff, const int32_t *zflat,
                        fw_test_result *out)
{
    if (m == 0) return FW_OK;
    FwBatch b;
    if (int rc = fwi_batch_upload(ctx, m, X, Y, zoff, zflat, b)) return rc;
    hipLaunchKernelGGL(fz64_test_batch_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)ctx->d_cor64, ctx->P.p,
                       (long long)m, (const int32_t *)b.dX, (const int32_t *)b.dY, (const long long *)b.dz, b.dzflat, fz64_zscale(ctx), b.dout);
    if (int rc = fwi_batch_finish(ctx, m, out)) return rc;
    if (ctx->P.n < ctx->n_obs_min_eff) fw_fill_no_power(out, m);  // tests.jl:254 / :111
    return FW_OK;
}

int fwi_fz64_segments(fw_ctx *ctx, int64_t nseg, const FwSeg *d_segs, const int32_t *d_acc, FwSegOut *d_out, FwPoolBuf &pb)
{
    if (nseg == 0) return FW_OK;
    FW_HIP(ctx, hipEventRecord(pb.ev0, pb.launch_stream));
    hipLaunchKernelGGL(fz64_subsets_kernel, dim3((unsigned)nseg), dim3(256), 0, pb.launch_stream, (const double *)ctx->d_cor64, ctx->P.p, d_segs,
                       d_acc, d_out, ctx->P.max_k, ctx->P.alpha, fz64_zscale(ctx), (long long)ctx->P.max_tests);
    FW_HIP(ctx, hipGetLastError());
    FW_HIP(ctx, hipEventRecord(pb.ev1, pb.launch_stream));
    return FW_OK;
}
