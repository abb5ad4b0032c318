// Normalisation front-end on the device: the count matrix goes to HBM once and comes out normalised,
// ready for fw_set_data_*.  Mirrors preprocess_data for a table without meta variables (reference src/preprocessing.jl):
//   filter_by_variance                  :367-409   zero-variance columns, then samples without reads
//   "fz"     clr_adapt                  :133-214   adaptive pseudo-counts (adaptive_pseudocount!) + centred log-ratio
//   "fz_nz"  clr_nz                     :192-207   log(x / geometric mean of the row's non-zeros), zeros stay zeros
//   "mi"     binary                     :475-490   presence / absence, columns with exactly two levels
//   "mi_nz"  binned_nz_clr              :217-291,492-521  clr_nz, then per column the tied (average) ranks of the non-zero entries,
//                                       rank / max rank, bin = floor(. / (1/2 + 1e-5)) + 1 (two bins, disc_method "median"), zeros stay 0;
//                                       columns whose non-zeros show exactly two bins
//   The two binned kinds ("mi_nz" and FW_NORM_TSS_BINNED below) take the reference's options (fw_norm_opts; discretize, :217-291): n_bins
//   (b = n_bins - 1 non-zero bins, 2 .. 61: step 1 / b + 1e-5, levels 1 .. b, a column is kept iff its non-zeros show exactly b levels,
//   :511-515), rank_method ("dense": the distinct keys numbered 1 .. d -- the sorted keys are compacted in place, nb_compact) and
//   disc_method ("mean", b = 2: key <= mean ? 1 : 2, the mean a pairwise sum over the sorted, zero-padded keys, nb_mean -- one number
//   on the host, in the dense and in the CSC form).  The defaults run the kernels' instantiation without options (OPTS = false): the rule
//   folded at compile time, the bits and the registers of the kernels before they took options.
// Arithmetic is Float64 like the reference (clrnorm converts to Matrix{Float64}); the continuous modes return Float32
// (convert_to_target_prec with prec = 32).  Layout: n samples x p variables, column-major, as Julia holds it; one thread
// per sample row and column chunk (adjacent lanes = adjacent samples: coalesced), chunk partials reduced in a fixed order.
// HBM-bound elementwise work: 4 B read per count and pass (3 passes) + 4 B written.
// Value type: every kernel that reads the table is a template over V = int32_t (counts: fw_normalize_counts*, the instantiation
// that runs for them as before) or double (real-valued tables: fw_normalize_abund*, 8 B read per cell and pass).  Both
// instantiations take the same expressions in the same order -- (double)v is the identity for V = double -- so a table of
// integers gives the same bits through either.
// Two further transforms, not test kinds (norm_mode of normalize_data, preprocessing.jl:660-684), under the same filters:
//   FW_NORM_TSS         rows            :348-361   x / (sum of the row over the kept columns)                 -> Float32
//   FW_NORM_TSS_BINNED  binned_nz_rows  :492-521   the ranks / bins of "mi_nz" with the TSS value as the key   -> Int32 {0, 1, 2}
// These stay in Float32 like the reference (check_convert_sparse converts the table to Float{prec} first, rownorm! divides by
// sum(X, dims=2)): x32 = (float)x; s_i = the Float32 sum of row i over the kept columns in ascending column order from +0.0f
// (a zero cell adds +0.0f, no bit changes: the CSC form adds the stored terms alone, in that order); out = x32 / s_i, one correctly
// rounded IEEE division (the Makefile passes no fast-math and no flush-to-zero flag).  Only + and / and no libm call: host,
// dense and CSC form agree to the bit, and so do the ties among the quotients, which decide the tied ranks.  The Float64 chunk
// partials of norm_row_stats_kernel are NOT s_i -- Float32 addition does not reassociate -- they only give the row filter.
// One more pass over the kept cells for s_i (4 | 8 B read per cell, 4 B written per row), then 4 | 8 B read + 4 B written per cell.
#include <rocprim/device/device_radix_sort.hpp>

#include "fw_csc.h"
#include "fw_internal.h"
#include "fw_norm_host.h"

namespace {

// What the value type is more than a type name for: the identities of min / max, the value check (a count is good when it is
// >= 0; a real value when it is >= 0 and finite -- anything else reads as -1, so that the one "smallest value < 0" test of the
// host refuses both; -0.0 is >= 0 and == 0: a zero), the words of the refusal, and which row sums count as equal (norm_row_params).
template <typename V> struct NormVal;
template <> struct NormVal<int32_t> {
    __host__ __device__ static int32_t vmax() { return 0x7fffffff; }
    __host__ __device__ static int32_t vmin() { return (int32_t)0x80000000; }
    __device__ static int32_t checked(int32_t v) { return v; }
    static const char *bad() { return "negative count"; }
    static double tie_rel(int) { return 0.0; }
};
template <> struct NormVal<double> {
    __host__ __device__ static double vmax() { return INFINITY; }
    __host__ __device__ static double vmin() { return -INFINITY; }
    __device__ static double checked(double v) { return (v >= 0.0 && v <= 1.7976931348623157e308) ? v : -1.0; }
    static const char *bad() { return "negative or non-finite (NaN, Inf) value"; }
    static double tie_rel(int pk) { return (double)pk * 0x1p-52; }
};

// per column: min and max over the samples (variance > 0 <=> min != max)
template <typename V>
__global__ __launch_bounds__(256) void norm_col_minmax_kernel(const V *__restrict__ x, int n, int p, V *__restrict__ cmin, V *__restrict__ cmax)
{
    __shared__ V s_lo[256], s_hi[256];
    const int j = blockIdx.x;
    V lo = NormVal<V>::vmax(), hi = NormVal<V>::vmin();
    for (int i = threadIdx.x; i < n; i += 256) {
        const V v = NormVal<V>::checked(x[(size_t)j * n + i]);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            s_lo[threadIdx.x] = s_lo[threadIdx.x + o] < s_lo[threadIdx.x] ? s_lo[threadIdx.x + o] : s_lo[threadIdx.x];
            s_hi[threadIdx.x] = s_hi[threadIdx.x + o] > s_hi[threadIdx.x] ? s_hi[threadIdx.x + o] : s_hi[threadIdx.x];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        cmin[j] = s_lo[0];
        cmax[j] = s_hi[0];
    }
}

// per (row, column chunk) over the kept columns: read sum, number of zeros, sum of log over the non-zeros, smallest non-zero
template <typename V>
__global__ __launch_bounds__(256) void norm_row_stats_kernel(const V *__restrict__ x, int n, const int32_t *__restrict__ cols, int pk,
                                                             double *__restrict__ rsum, int32_t *__restrict__ rzero,
                                                             double *__restrict__ rlog, V *__restrict__ rmin)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = blockIdx.y;
    const int per = (pk + NORM_CHUNKS - 1) / NORM_CHUNKS;
    const int j0 = c * per, j1 = (j0 + per) < pk ? (j0 + per) : pk;
    double s = 0.0, sl = 0.0;
    int nz = 0;
    V mn = NormVal<V>::vmax();
    for (int q = j0; q < j1; ++q) {
        const V v = x[(size_t)cols[q] * n + i];
        s += (double)v;
        if (v == 0) {
            ++nz;
        } else {
            sl += log((double)v);
            mn = v < mn ? v : mn;
        }
    }
    rsum[(size_t)c * n + i] = s;
    rzero[(size_t)c * n + i] = nz;
    rlog[(size_t)c * n + i] = sl;
    rmin[(size_t)c * n + i] = mn;
}

// TSS: per sample the Float32 sum over the kept columns, left to right from +0.0f (one thread per sample, adjacent lanes on
// adjacent samples: coalesced; the order IS the result, so no chunks).  rsum32[i] for every input row i.
template <typename V>
__global__ __launch_bounds__(256) void norm_row_tss_kernel(const V *__restrict__ x, int n, const int32_t *__restrict__ cols, int pk,
                                                           float *__restrict__ rsum32)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int q = 0; q < pk; ++q) s += (float)x[(size_t)cols[q] * n + i];
    rsum32[i] = s;
}

// TSS: out[r][q] = (float)x / rsum32[row] for kept rows r and kept columns q (column-major n_out x p_out)
template <typename V>
__global__ __launch_bounds__(256) void norm_tss_out_kernel(const V *__restrict__ x, int n, const int32_t *__restrict__ rows, int nk,
                                                           const int32_t *__restrict__ cols, int pk, const float *__restrict__ rsum32,
                                                           float *__restrict__ out)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nk) return;
    const int i = rows[r];
    const float s = rsum32[i];
    for (int q = blockIdx.y; q < pk; q += gridDim.y) out[(size_t)q * nk + r] = (float)x[(size_t)cols[q] * n + i] / s;
}

// out[r][q] for kept rows r and kept columns q (column-major n_out x p_out)
//   mode 0 (clr_adapt): log(x' / g_r), x' = x or the row's pseudo-count, g_r = exp(mean log x')
//   mode 1 (clr_nz):    x == 0 ? 0 : log(x / g_r), g_r = exp(mean log of the non-zeros)
template <typename V>
__global__ __launch_bounds__(256) void norm_clr_out_kernel(const V *__restrict__ x, int n, const int32_t *__restrict__ rows, int nk,
                                                           const int32_t *__restrict__ cols, int pk, const double *__restrict__ pseudo,
                                                           const double *__restrict__ gmean, int mode, float *__restrict__ out)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nk) return;
    for (int q = blockIdx.y; q < pk; q += gridDim.y) {  // (grid.y is capped at NORM_GRID_Y: tables with more kept columns loop)
        const V v = x[(size_t)cols[q] * n + rows[r]];
        double o;
        if (mode == 0)
            o = log((v == 0 ? pseudo[r] : (double)v) / gmean[r]);
        else
            o = v == 0 ? 0.0 : log((double)v / gmean[r]);
        out[(size_t)q * nk + r] = (float)o;
    }
}

template <typename V>
__global__ __launch_bounds__(256) void norm_binary_out_kernel(const V *__restrict__ x, int n, const int32_t *__restrict__ rows, int nk,
                                                              const int32_t *__restrict__ cols, int pk, int32_t *__restrict__ out)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nk) return;
    for (int q = blockIdx.y; q < pk; q += gridDim.y) out[(size_t)q * nk + r] = x[(size_t)cols[q] * n + rows[r]] != 0 ? 1 : 0;
}

// per kept column over the kept rows: does it hold both a zero and a non-zero?
template <typename V>
__global__ __launch_bounds__(256) void norm_col_levels_kernel(const V *__restrict__ x, int n, const int32_t *__restrict__ rows, int nk,
                                                              const int32_t *__restrict__ cols, int pk, int32_t *__restrict__ two)
{
    __shared__ int s_z, s_nz;
    const int q = blockIdx.x;
    if (threadIdx.x == 0) s_z = s_nz = 0;
    __syncthreads();
    int z = 0, nzz = 0;
    for (int r = threadIdx.x; r < nk; r += 256) {
        const V v = x[(size_t)cols[q] * n + rows[r]];
        z |= v == 0;
        nzz |= v != 0;
    }
    if (z) s_z = 1;
    if (nzz) s_nz = 1;
    __syncthreads();
    if (threadIdx.x == 0) two[q] = s_z && s_nz;
}

// binned_nz_clr, one workgroup per kept column: the clr_nz values log(x / g_row) of the column's non-zero entries (kept rows) go
// to LDS and are sorted there (bitonic, +inf padding); an entry's tied rank is then (#smaller) + (#equal + 1) / 2 from two binary
// searches, the largest rank m - (e_max - 1) / 2, and bin = floor((rank / max rank) / (1/2 + 1e-5)) + 1 exactly as discretize()
// computes it in Float64 (preprocessing.jl:238-265 with n_bins - 1 = 2 for the non-zeros, :267-291).  two[q] = the non-zeros show
// both bins: every thread collects the levels it wrote as bits of a 64-bit mask, the masks are OR-ed over the workgroup (nb_all_levels)
// and two[q] = (popcount == b).  With options (OPTS: b, rank_dense, disc_mean at run time) the step is 1 / b + 1e-5, the ranks are
// searched among the distinct keys after nb_compact, or the level comes from nb_mean's threshold.  LDS: the keys (dynamic, up to
// 128 KB) + 196 bytes of statics (s_cnt, the 16 wave totals of the compaction's scan, the 16 wave masks) of gfx950's 160 KB.
// The keys live in LDS, 8 bytes per padded entry, up to 16 384 kept rows; beyond (r04: preprocessing.jl:217-291 has no
// bound) in a slice of device memory per workgroup (gkeys, M doubles each: the same bitonic network, its passes through L2
// instead of LDS -- the stores of a pass are visible to the workgroup's other wavefronts behind the barrier, one L1 per CU), the
// workgroups striding over the columns so that the scratch stays at gridDim.x * M doubles.
#define NORM_BIN_MAX 16384

// The sort keys of one workgroup: in LDS plain accesses; in device memory relaxed agent-scope accesses (they bypass the per-CU
// vector cache, whose lines another wavefront's store does not refresh) and a device-scope fence in front of every barrier.
struct NbKeys {
    double *k;
    bool glob;
    __device__ double ld(int i) const
    {
        return glob ? __longlong_as_double(__hip_atomic_load((const long long *)&k[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : k[i];
    }
    __device__ void st(int i, double v) const
    {
        if (glob)
            __hip_atomic_store((long long *)&k[i], __double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else
            k[i] = v;
    }
    __device__ void sync() const
    {
        if (glob) __threadfence();
        __syncthreads();
    }
};

// The rank / bin code of binned_nz_clr, shared by the dense and the CSC form (all nt threads of the workgroup call nb_pad_sort).
// keys[0 .. m) are filled and synchronised: pad to M (a power of two) with +inf and sort ascending (bitonic).
__device__ inline void nb_pad_sort(const NbKeys &K, int m, int M, int tid, int nt)
{
    for (int i = m + tid; i < M; i += nt) K.st(i, INFINITY);
    K.sync();
    for (int k = 2; k <= M; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < M; i += nt) {
                const int l = i ^ j;
                if (l > i) {
                    const double a = K.ld(i), b = K.ld(l);
                    const bool up = (i & k) == 0;
                    if (up ? (a > b) : (a < b)) {
                        K.st(i, b);
                        K.st(l, a);
                    }
                }
            }
            K.sync();
        }
}

// the largest tied rank among the m sorted keys: m - (e_max - 1) / 2
__device__ inline double nb_rank_max(const NbKeys &K, int m)
{
    if (m <= 0) return 1.0;
    const double top = K.ld(m - 1);
    int lo = 0, hi = m;  // first index with key >= top
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (K.ld(mid) < top)
            lo = mid + 1;
        else
            hi = mid;
    }
    return (double)m - ((double)(m - lo) - 1.0) / 2.0;
}

// What the options of the binned kinds (NormOpts) come to for one column, the same in every thread of the workgroup: b non-zero bins;
// m_eff = how many of the keys the ranks are searched in (tied: the m sorted keys; dense: the d distinct ones nb_compact left), rmax the
// largest rank (dense: d); mean: the "mean" rule with its threshold instead of ranks.
struct NbRule {
    int b, m_eff;
    bool dense, mean;
    double rmax, thresh;
};

// level of the value c (one of the column's keys).  "median": rank / max rank, level = floor(. / (1 / b + 1e-5)) + 1, in 1 .. b -- the
// tied rank (#smaller) + (#equal + 1) / 2 among the sorted keys, or the dense rank (#smaller distinct) + 1 among the distinct ones;
// b = 2 gives the step 1/2 + 1e-5 to the bit.  "mean": c <= mean ? 1 : 2.
__device__ inline int nb_bin(const NbKeys &K, const NbRule &R, double c)
{
    if (R.mean) return c <= R.thresh ? 1 : 2;
    const double step = (1.0 / (double)R.b) + 1e-5;
    int lo = 0, hi = R.m_eff;
    while (lo < hi) {  // #smaller
        const int mid = (lo + hi) >> 1;
        if (K.ld(mid) < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    double rank = (double)(lo + 1);
    if (!R.dense) {
        int lo2 = lo, hi2 = R.m_eff;
        while (lo2 < hi2) {  // first index with key > c
            const int mid = (lo2 + hi2) >> 1;
            if (K.ld(mid) <= c)
                lo2 = mid + 1;
            else
                hi2 = mid;
        }
        rank = (double)lo + ((double)(lo2 - lo) + 1.0) / 2.0;
    }
    return (int)floor((rank / R.rmax) / step) + 1;
}

// Dense ranks: the m sorted keys are compacted in place to the d distinct ones (-> d; what lies in [d, m) afterwards is stale and not
// read again).  Tile by tile of nt * NB_RUN keys, in ascending order: every thread reads its contiguous run of NB_RUN keys (and the run's
// predecessor) into registers and counts the keys that differ from their predecessor; wave scan (shuffles) + the wave totals through
// s_part give every run its place among the distinct keys -- the barrier of that scan is also the one behind the tile's last read;
// then each thread writes its distinct keys, and a second barrier (with the fence of the device-memory placement) closes the tile.
// A destination never exceeds its source index (at most i distinct keys lie before key i), so a tile's writes stay below every key
// that is still unread.  All nt threads call it (nt a multiple of 64, at most 1 024); s_part: 16 ints of LDS.
#define NB_RUN 8
__device__ inline int nb_compact(const NbKeys &K, int m, int tid, int nt, int *s_part)
{
    const int lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    int d = 0;
    for (int base = 0; base < m; base += nt * NB_RUN) {
        const int i0 = base + tid * NB_RUN;
        double key[NB_RUN];
        double prev = (i0 > 0 && i0 < m) ? K.ld(i0 - 1) : 0.0;
        unsigned first = 0;  // bit u: key i0 + u is the first of its value
        int cnt = 0;
#pragma unroll
        for (int u = 0; u < NB_RUN; ++u) {
            key[u] = 0.0;
            if (i0 + u < m) {
                key[u] = K.ld(i0 + u);
                if (i0 + u == 0 || key[u] != prev) {
                    first |= 1u << u;
                    ++cnt;
                }
                prev = key[u];
            }
        }
        int incl = cnt;  // inclusive scan over the wavefront
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o, 64);
            if (lane >= o) incl += up;
        }
        if (lane == 63) s_part[wave] = incl;
        __syncthreads();  // (every key of the tile has been read)
        int dst = d + incl - cnt, total = 0;
        for (int w = 0; w < nw; ++w) {
            const int t = s_part[w];
            if (w < wave) dst += t;
            total += t;
        }
#pragma unroll
        for (int u = 0; u < NB_RUN; ++u)
            if (first & (1u << u)) K.st(dst++, key[u]);
        d += total;
        K.sync();  // (the writes are visible; s_part is free for the next tile)
    }
    return d;
}

// The "mean" rule's threshold: the m sorted keys, padded with +0.0 to P = the next power of two, added pairwise level by level
// (a[2i] + a[2i+1]), divided by m.  In place over the keys, which the rule does not read again: level s leaves its sums at the multiples of 2s,
// each written by the one thread that read it, its partner (+ s) written by nobody at that level; one barrier per level.
__device__ inline double nb_mean(const NbKeys &K, int m, int tid, int nt)
{
    if (m <= 0) return 0.0;
    int P = 1;
    while (P < m) P <<= 1;
    for (int i = m + tid; i < P; i += nt) K.st(i, 0.0);  // (+inf padding of the sort -> +0.0; P <= the padded length of the sort)
    K.sync();
    for (int s = 1; s < P; s <<= 1) {
        for (int i = tid; i < P / (2 * s); i += nt) K.st(2 * s * i, K.ld(2 * s * i) + K.ld(2 * s * i + s));
        K.sync();
    }
    return K.ld(0) / (double)m;
}

// The column's rule from its m sorted keys (all nt threads; the keys are synchronised on entry and on return).  OPTS = false is the
// instantiation of the default options -- two bins, tied ranks, "median" -- with the rule folded at compile time: the code, and the
// registers, the kernels had before they took options; dense and mean are not looked at (the host passes b = 2, which the column rule
// counts the levels against).  The predecessor nb_compact reads across a tile's edge is still the original key: the tile before wrote
// up to there only if all its keys were distinct, and then wrote each key onto itself.
template <bool OPTS> __device__ inline NbRule nb_rule(const NbKeys &K, int m, int b, int dense, int mean, int tid, int nt, int *s_part)
{
    if (!OPTS) return NbRule{2, m, false, false, nb_rank_max(K, m), 0.0};
    NbRule R{b, m, dense != 0, mean != 0, 1.0, 0.0};
    if (R.mean) {
        R.thresh = nb_mean(K, m, tid, nt);
    } else if (R.dense) {
        R.m_eff = nb_compact(K, m, tid, nt, s_part);
        R.rmax = R.m_eff > 0 ? (double)R.m_eff : 1.0;
    } else {
        R.rmax = nb_rank_max(K, m);
    }
    return R;
}

// The levels the workgroup's threads saw (bit l: level l) -> true when they are exactly b: OR over the wavefront by shuffles, the wave
// results through s_wmask (16 words of LDS), counted by every thread alike.  Ends behind a barrier; s_wmask is free after the next one.
__device__ inline bool nb_all_levels(unsigned long long seen, int b, int tid, int nt, unsigned long long *s_wmask)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) seen |= __shfl_xor(seen, o, 64);
    if ((tid & 63) == 0) s_wmask[tid >> 6] = seen;
    __syncthreads();
    unsigned long long all = 0;
    for (int w = 0; w < (nt >> 6); ++w) all |= s_wmask[w];
    return __popcll(all) == b;
}

// The sort key of a non-zero entry v in kept row r = input row i.  binned_nz_clr: its clr_nz value.  TSS (binned_nz_rows): its
// Float32 quotient, widened -- which keeps order and ties.
template <bool TSS, typename V>
__device__ inline double nb_key(V v, const double *__restrict__ gmean, int r, const float *__restrict__ rsum32, int i)
{
    if (TSS) return (double)((float)v / rsum32[i]);
    return log((double)v / gmean[r]);
}

template <typename V, bool TSS, bool OPTS>
__global__ __launch_bounds__(1024) void norm_binned_kernel(const V *__restrict__ x, int n, const int32_t *__restrict__ rows, int nk,
                                                           const int32_t *__restrict__ cols, int pk, const double *__restrict__ gmean,
                                                           const float *__restrict__ rsum32, int32_t *__restrict__ out,
                                                           int32_t *__restrict__ two, int M, double *gkeys, int nb, int rank_dense,
                                                           int disc_mean)
{
    extern __shared__ double s_key_lds[];
    __shared__ int s_cnt, s_part[16];
    __shared__ unsigned long long s_wmask[16];
    const int tid = threadIdx.x;
    const NbKeys K{gkeys ? gkeys + (size_t)blockIdx.x * (size_t)M : s_key_lds, gkeys != nullptr};
  for (int q = blockIdx.x; q < pk; q += gridDim.x) {
    const V *col = x + (size_t)cols[q] * n;
    __syncthreads();  // (the previous column's last readers of the keys / s_cnt / s_wmask)
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int r = tid; r < nk; r += 1024) {
        const V v = col[rows[r]];
        if (v != 0) K.st(atomicAdd(&s_cnt, 1), nb_key<TSS>(v, gmean, r, rsum32, rows[r]));  // order does not matter: sorted below
    }
    K.sync();
    const int m = s_cnt;
    nb_pad_sort(K, m, M, tid, 1024);
    const NbRule R = nb_rule<OPTS>(K, m, nb, rank_dense, disc_mean, tid, 1024, s_part);
    unsigned long long seen = 0;
    for (int r = tid; r < nk; r += 1024) {
        const V v = col[rows[r]];
        int bin = 0;
        if (v != 0) {
            bin = nb_bin(K, R, nb_key<TSS>(v, gmean, r, rsum32, rows[r]));  // the same operations as above: the same bits
            seen |= 1ull << bin;
        }
        out[(size_t)q * nk + r] = bin;
    }
    const bool all = nb_all_levels(seen, nb, tid, 1024, s_wmask);
    if (tid == 0) two[q] = all;
  }
}

// dst column q2 = src column sel[q2] (nk entries each)
__global__ __launch_bounds__(256) void norm_gather_cols_kernel(const int32_t *__restrict__ src, const int32_t *__restrict__ sel, int nk, int pk,
                                                               int32_t *__restrict__ dst)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nk) return;
    for (int q = blockIdx.y; q < pk; q += gridDim.y) dst[(size_t)q * nk + r] = src[(size_t)sel[q] * nk + r];
}

#define NORM_GRID_Y 65535  // HIP's limit on grid.y: the per-column output kernels loop beyond it
// ---- the host half: a driver is a sequence of stages (the filters: kept columns, then row totals -> kept samples; the output), each a
// function that returns on error; device scratch lives in FwDevArray, the rules without device code in fw_norm_host.h.  NormCall: what the
// stages share (fn: the entry point's name, for the messages) and leave for the next: kept columns (input ids), kept samples, TSS row sums.
struct NormCall {
    const char *fn;
    int kind;
    NormKind K;
    int n;
    uint8_t *row_mask, *col_mask;
    NormOpts O;  // the options of the binned kinds (fw_norm_opts, checked: norm_call_check)
    std::vector<int32_t> cols;
    NormRows R;
    FwDevArray<int32_t> d_cols;
    FwDevArray<float> d_s32;
    bool dev_out = false;  // the *_dev entry points: out_f32 / out_i32 are the caller's device buffers, written by the output kernels
};

dim3 norm_out_grid(int nk, int pk) { return dim3((nk + 255) / 256, std::min(pk, NORM_GRID_Y)); }
int norm_all_constant(const char *fn) { return fw_fail(nullptr, FW_ERR_ARG, "%s: every column is constant", fn); }
// the kind's own filter (norm_keep_columns) left nothing, or -- FW_FZ -- the pseudo-counts did; the binned kinds away from two non-zero
// bins say how many levels were asked for
int norm_none_left(const NormCall &c)
{
    if (c.K.binned && c.O.b != 2) return fw_fail(nullptr, FW_ERR_ARG, "%s: no column whose non-zero abundances show all %d non-zero levels (n_bins = %d)", c.fn, c.O.b, c.O.b + 1);
    return fw_fail(nullptr, FW_ERR_ARG, "%s: %s", c.fn, c.K.none_left);
}
// kind and options of a call, before any device call: an unknown kind, or an option the kind does not take (norm_opts_check's words)
int norm_call_check(NormCall &c, const fw_norm_opts *opts)
{
    if (!c.K.known) return fw_fail(nullptr, FW_ERR_ARG, "%s: unknown kind %d", c.fn, c.kind);
    if (const char *no = norm_opts_check(opts, c.K, c.O)) return fw_fail(nullptr, FW_ERR_ARG, "%s: fw_norm_opts: %s", c.fn, no);
    return FW_OK;
}

// row totals -> kept samples, pseudo-counts, geometric means and the TSS divisors (norm_row_params), a refusal in words
int norm_rows(NormCall &c, double tie_rel, const NormTotals &T, const std::vector<float> &s32)
{
    const NormRefusal no = norm_row_params(c.kind, c.n, (int)c.cols.size(), tie_rel, T, c.K.tss ? &s32 : nullptr, c.row_mask, c.R);
    if (!no.reason) return FW_OK;
    if (no.sample < 0) return fw_fail(nullptr, FW_ERR_ARG, "%s: %s", c.fn, no.reason);
    return fw_fail(nullptr, FW_ERR_ARG, "%s: the Float32 sum of sample %d is %s: total-sum scaling needs values within the Float32 range", c.fn, no.sample, no.reason);
}

// The launch shape of the binned kernels.  M = the padded length of the longest run of keys: dense the kept samples, on 1 024 threads;
// CSC the longest kept column, on 256 | 1 024 threads (csc_binned_kernel).  The keys in LDS up to NORM_BIN_MAX, beyond in device memory.
struct NormBinShape {
    int M = 2, grid = 0, threads = 0;
    FwDevArray<double> keys;  // (nullptr: the keys live in LDS, M doubles)
    size_t lds() const { return keys.get() ? 0 : sizeof(double) * (size_t)M; }
};
int norm_bin_shape(const void *kernel, long long longest, int pk, bool dense, NormBinShape &B)
{
    while (B.M < longest) B.M <<= 1;
    const bool keys_in_lds = B.M <= NORM_BIN_MAX;  // beyond: one slice of device memory per workgroup
    B.grid = keys_in_lds ? pk : std::min(pk, 1024);
    B.threads = dense || B.M > 2048 ? 1024 : 256;  // short columns (the HE case): more workgroups per CU instead of idle lanes
    if (!keys_in_lds) FW_HIP(nullptr, B.keys.alloc((size_t)B.M * (size_t)B.grid));
    FW_HIP(nullptr, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * NORM_BIN_MAX)));
    return FW_OK;
}

// The dense filters.  Columns: the value check and var(data, dims=1) .> 0.  Row totals over the kept columns: the chunk partials, reduced
// on the host; TSS: the Float32 row sums in their own order (the Float64 partials give the row filter only).
template <typename V> int dense_filters(NormCall &c, const V *d_x, int p)
{
    const int n = c.n;
    const size_t cn = (size_t)NORM_CHUNKS * n;
    FwDevArray<V> d_cmin, d_cmax, d_rmin;
    FwDevArray<double> d_rsum, d_rlog;
    FwDevArray<int32_t> d_rzero;
    std::vector<V> cmin((size_t)p), cmax((size_t)p), rmin(cn);
    std::vector<double> rsum(cn), rlog(cn);
    std::vector<int32_t> rzero(cn);
    std::vector<float> s32(c.K.tss ? (size_t)n : 0);
    FW_HIP(nullptr, d_cmin.alloc((size_t)p));
    FW_HIP(nullptr, d_cmax.alloc((size_t)p));
    hipLaunchKernelGGL(norm_col_minmax_kernel<V>, dim3(p), dim3(256), 0, 0, d_x, n, p, d_cmin.get(), d_cmax.get());
    FW_HIP(nullptr, hipGetLastError());
    FW_HIP(nullptr, d_cmin.download(cmin));
    FW_HIP(nullptr, d_cmax.download(cmax));
    for (int j = 0; j < p; ++j) {
        if (cmin[j] < 0) return fw_fail(nullptr, FW_ERR_ARG, "%s: %s in column %d", c.fn, NormVal<V>::bad(), j);
        c.col_mask[j] = cmin[j] != cmax[j];  // var(data, dims=1) .> 0
        if (c.col_mask[j]) c.cols.push_back(j);
    }
    const int pk = (int)c.cols.size();
    if (pk == 0) return norm_all_constant(c.fn);
    FW_HIP(nullptr, c.d_cols.upload(c.cols));
    FW_HIP(nullptr, d_rsum.alloc(cn));
    FW_HIP(nullptr, d_rlog.alloc(cn));
    FW_HIP(nullptr, d_rzero.alloc(cn));
    FW_HIP(nullptr, d_rmin.alloc(cn));
    hipLaunchKernelGGL(norm_row_stats_kernel<V>, dim3((n + 255) / 256, NORM_CHUNKS), dim3(256), 0, 0, d_x, n, c.d_cols.get(), pk, d_rsum.get(), d_rzero.get(), d_rlog.get(), d_rmin.get());
    FW_HIP(nullptr, hipGetLastError());
    FW_HIP(nullptr, d_rsum.download(rsum));
    FW_HIP(nullptr, d_rlog.download(rlog));
    FW_HIP(nullptr, d_rzero.download(rzero));
    FW_HIP(nullptr, d_rmin.download(rmin));
    if (c.K.tss) {
        FW_HIP(nullptr, c.d_s32.alloc((size_t)n));
        hipLaunchKernelGGL(norm_row_tss_kernel<V>, dim3((n + 255) / 256), dim3(256), 0, 0, d_x, n, c.d_cols.get(), pk, c.d_s32.get());
        FW_HIP(nullptr, hipGetLastError());
        FW_HIP(nullptr, c.d_s32.download(s32));
    }
    return norm_rows(c, NormVal<V>::tie_rel(pk), norm_reduce_chunks(n, rsum, rlog, rzero, rmin), s32);
}

// dense output: the kind's transform over the kept cells -> out_i32 | out_f32 (column-major, kept samples x the columns left in cols):
// host buffers the result is downloaded into, or (c.dev_out) device buffers of n p elements the output kernels write themselves
template <typename V> int dense_output(NormCall &c, const V *d_x, float *out_f32, int32_t *out_i32)
{
    const int n = c.n, nk = (int)c.R.rows.size(), pk = (int)c.cols.size();
    FwDevArray<int32_t> d_rows, d_two, d_oi, d_tmp, d_sel;
    FwDevArray<double> d_pseudo, d_g;
    FwDevArray<float> d_of;
    std::vector<int32_t> two((size_t)pk);
    FW_HIP(nullptr, d_rows.upload(c.R.rows));
    float *of = out_f32;
    int32_t *oi = out_i32;
    if (!c.K.i32 && !c.dev_out) {
        FW_HIP(nullptr, d_of.alloc((size_t)nk * pk));
        of = d_of.get();
    }
    if (c.K.i32 && !c.K.binned) {  // FW_MI: presabs_norm! + columns with exactly two levels among the kept samples
        FW_HIP(nullptr, d_two.alloc((size_t)pk));
        hipLaunchKernelGGL(norm_col_levels_kernel<V>, dim3(pk), dim3(256), 0, 0, d_x, n, d_rows.get(), nk, c.d_cols.get(), pk, d_two.get());
        FW_HIP(nullptr, hipGetLastError());
        FW_HIP(nullptr, d_two.download(two));
        if (norm_keep_columns(two, c.cols, c.col_mask).empty()) return norm_none_left(c);
        const int pf = (int)c.cols.size();
        FW_HIP(nullptr, hipMemcpy(c.d_cols.get(), c.cols.data(), sizeof(int32_t) * pf, hipMemcpyHostToDevice));
        if (!c.dev_out) {
            FW_HIP(nullptr, d_oi.alloc((size_t)nk * pf));
            oi = d_oi.get();
        }
        hipLaunchKernelGGL(norm_binary_out_kernel<V>, norm_out_grid(nk, pf), dim3(256), 0, 0, d_x, n, d_rows.get(), nk, c.d_cols.get(), pf, oi);
    } else if (c.K.binned) {  // every kept column is binned, then the columns that show both bins are gathered
        const auto binned = c.O.plain() ? (!c.K.tss ? norm_binned_kernel<V, false, false> : norm_binned_kernel<V, true, false>)  // (the key: nb_key)
                                        : (!c.K.tss ? norm_binned_kernel<V, false, true> : norm_binned_kernel<V, true, true>);
        NormBinShape B;
        if (int rc = norm_bin_shape((const void *)binned, nk, pk, true, B)) return rc;
        FW_HIP(nullptr, d_g.upload(c.R.g));
        FW_HIP(nullptr, d_two.alloc((size_t)pk));
        FW_HIP(nullptr, d_tmp.alloc((size_t)nk * pk));
        hipLaunchKernelGGL(binned, dim3(B.grid), dim3(B.threads), B.lds(), 0, d_x, n, d_rows.get(), nk, c.d_cols.get(), pk, d_g.get(), c.d_s32.get(), d_tmp.get(), d_two.get(), B.M, B.keys.get(), c.O.b, (int)c.O.dense, (int)c.O.mean);
        FW_HIP(nullptr, hipGetLastError());
        FW_HIP(nullptr, d_two.download(two));
        const std::vector<int32_t> sel = norm_keep_columns(two, c.cols, c.col_mask);
        const int pf = (int)sel.size();
        if (pf == 0) return norm_none_left(c);
        FW_HIP(nullptr, d_sel.upload(sel));
        if (!c.dev_out) {
            FW_HIP(nullptr, d_oi.alloc((size_t)nk * pf));
            oi = d_oi.get();
        }
        hipLaunchKernelGGL(norm_gather_cols_kernel, norm_out_grid(nk, pf), dim3(256), 0, 0, d_tmp.get(), d_sel.get(), nk, pf, oi);
    } else if (c.K.tss) {
        hipLaunchKernelGGL(norm_tss_out_kernel<V>, norm_out_grid(nk, pk), dim3(256), 0, 0, d_x, n, d_rows.get(), nk, c.d_cols.get(), pk, c.d_s32.get(), of);
    } else {
        FW_HIP(nullptr, d_pseudo.upload(c.R.pseudo));
        FW_HIP(nullptr, d_g.upload(c.R.g));
        hipLaunchKernelGGL(norm_clr_out_kernel<V>, norm_out_grid(nk, pk), dim3(256), 0, 0, d_x, n, d_rows.get(), nk, c.d_cols.get(), pk, d_pseudo.get(), d_g.get(), c.K.clr_mode, of);
    }
    FW_HIP(nullptr, hipGetLastError());
    if (c.dev_out) {  // (the caller reads its buffer at once)
        FW_HIP(nullptr, hipStreamSynchronize(0));
        return FW_OK;
    }
    if (c.K.i32) FW_HIP(nullptr, d_oi.download(out_i32, (size_t)nk * c.cols.size()));
    if (!c.K.i32) FW_HIP(nullptr, d_of.download(out_f32, (size_t)nk * c.cols.size()));
    return FW_OK;
}

// The dense front-end for either value type (fn: the entry point's name, for the messages).  dev: the *_dev form -- counts and the
// output buffer are device memory of `device` (asked of the runtime before anything reads them); the table is borrowed, not uploaded,
// and the output is written in place, not downloaded.  The stages and their kernels are the same, so the bits are.
template <typename V>
int norm_dense(const char *fn, int32_t device, int32_t kind, int32_t n, int32_t p, const V *counts, float *out_f32, int32_t *out_i32,
               uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, const fw_norm_opts *opts, bool dev = false)
{
    if (!counts || !row_mask || !col_mask || !n_out || !p_out || n <= 0 || p <= 0) return fw_fail(nullptr, FW_ERR_ARG, "%s: invalid argument", fn);
    NormCall c{fn, kind, norm_kind(kind), n, row_mask, col_mask};
    if (int rc = norm_call_check(c, opts)) return rc;
    if (c.K.i32 ? !out_i32 : !out_f32) return fw_fail(nullptr, FW_ERR_ARG, "%s: missing output buffer", fn);
    c.dev_out = dev;
    if (dev && !fw_is_dev_ptr(counts, device)) return fw_fail(nullptr, FW_ERR_ARG, "%s: the table is not device memory of device %d", fn, device);
    if (dev && !fw_is_dev_ptr(c.K.i32 ? (const void *)out_i32 : (const void *)out_f32, device))
        return fw_fail(nullptr, FW_ERR_ARG, "%s: the output buffer is not device memory of device %d", fn, device);
    FwDevArray<V> d_x;
    FW_HIP(nullptr, hipSetDevice(device));
    if (!dev) FW_HIP(nullptr, d_x.upload(counts, (size_t)n * p));
    const V *x = dev ? counts : d_x.get();
    if (int rc = dense_filters(c, x, p)) return rc;
    if (int rc = dense_output(c, x, out_f32, out_i32)) return rc;
    *n_out = (int32_t)c.R.rows.size();
    *p_out = (int32_t)c.cols.size();
    return FW_OK;
}

}  // namespace

// The entry points without options forward to their _opts siblings with NULL (the defaults); a refusal names the sibling.
extern "C" int fw_normalize_counts_opts(int32_t device, int32_t kind, int32_t n, int32_t p, const int32_t *counts, float *out_f32,
                                        int32_t *out_i32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out,
                                        const fw_norm_opts *opts)
{
    return norm_dense<int32_t>(opts ? "fw_normalize_counts_opts" : "fw_normalize_counts", device, kind, n, p, counts, out_f32, out_i32, row_mask, col_mask, n_out, p_out, opts);
}

extern "C" int fw_normalize_counts(int32_t device, int32_t kind, int32_t n, int32_t p, const int32_t *counts, float *out_f32,
                                   int32_t *out_i32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out)
{
    return fw_normalize_counts_opts(device, kind, n, p, counts, out_f32, out_i32, row_mask, col_mask, n_out, p_out, nullptr);
}

extern "C" int fw_normalize_abund_opts(int32_t device, int32_t kind, int32_t n, int32_t p, const double *values, float *out_f32,
                                       int32_t *out_i32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out,
                                       const fw_norm_opts *opts)
{
    return norm_dense<double>(opts ? "fw_normalize_abund_opts" : "fw_normalize_abund", device, kind, n, p, values, out_f32, out_i32, row_mask, col_mask, n_out, p_out, opts);
}

// The *_dev forms: the table and the output buffer in device memory (include/flashweave_amd.h); opts == NULL means the defaults.
extern "C" int fw_normalize_counts_dev(int32_t device, int32_t kind, int32_t n, int32_t p, const int32_t *d_counts, float *d_out_f32,
                                       int32_t *d_out_i32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out,
                                       const fw_norm_opts *opts)
{
    return norm_dense<int32_t>("fw_normalize_counts_dev", device, kind, n, p, d_counts, d_out_f32, d_out_i32, row_mask, col_mask, n_out, p_out, opts, true);
}

extern "C" int fw_normalize_abund_dev(int32_t device, int32_t kind, int32_t n, int32_t p, const double *d_values, float *d_out_f32,
                                      int32_t *d_out_i32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out,
                                      const fw_norm_opts *opts)
{
    return norm_dense<double>("fw_normalize_abund_dev", device, kind, n, p, d_values, d_out_f32, d_out_i32, row_mask, col_mask, n_out, p_out, opts, true);
}

extern "C" int fw_normalize_abund(int32_t device, int32_t kind, int32_t n, int32_t p, const double *values, float *out_f32,
                                  int32_t *out_i32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out)
{
    return fw_normalize_abund_opts(device, kind, n, p, values, out_f32, out_i32, row_mask, col_mask, n_out, p_out, nullptr);
}

// ---- the same front-end on a CSC count table (fw_normalize_counts_csc) ---------------------------------------------------------
// The table stays sparse from the caller's triple to the output triple: the work is O(nnz) (FW_FZ: plus its dense output).
// Bytes per entry: Int32 counts | Float64 values (fw_normalize_abund_csc).
//   csc_col_scan_kernel    one wavefront per column: structure and value check, min / max with the implicit zeros counted (the
//                          variance filter), and the payload of every entry for the sort                             12 | 20 B / entry
//   rocprim radix sort     stable, by row: the CSR view; inside a row the entries keep their ascending column order  ~24 | ~16 B / entry and pass
//   csc_row_stats_kernel   one thread per row over its CSR run: the sums of norm_row_stats_kernel in its order       12 | 20 B / entry
//   csc_binned_kernel      one workgroup per kept column: norm_binned_kernel on the column's stored run              16 | 24 B / entry
//   csc_emit_kernel        one wavefront per output column: renumbered rows + values                                 16 | 20 B / entry
//   csc_adapt_*_kernel     FW_FZ: the dense clr_adapt matrix, pseudo-count cells first, stored entries over them
// The payload of the sort (CscPay): a count travels beside its column in one 64-bit word, column << 32 | count.  A Float64 value
// does not fit beside its column, so for V = double the payload is the entry's index (32 bits: nnz < 2^31), the scan writes the
// entry's column into a uint32 of its own (ecol), and the row pass gathers value and column through the sorted index: 8 B / entry
// (index + ecol) where the packed word takes 8, and a sort that moves 8 B per entry and pass instead of 12; the row pass pays with
// two gathers (12 B / entry, uncoalesced).  Searching colptr for the column instead would save ecol's 4 B and cost log2(p) loads.
// Bit-identity with the dense form: norm_row_stats_kernel adds a row's terms chunk by chunk of the kept-column index and the host adds
// the 64 chunk partials in chunk order, each from 0.0.  An absent entry adds +0.0 to the read sum and nothing to the log sum, and
// a chunk without entries contributes a partial of +0.0: neither changes a bit, so adding the stored terms in column order with a
// fresh partial at every chunk boundary gives the same Float64 totals.  The per-row parameters come from the same host code
// (norm_row_params), the values from the same device expressions.
// The TSS kinds: csc_row_stats_kernel also adds the run's values as Float32, in the run's order -- the stable sort keeps a row's
// entries in ascending column order, so this is norm_row_tss_kernel's sum without its +0.0f terms (4 B written per row);
// csc_binned_kernel takes the Float32 quotient as its key, csc_emit_kernel writes it (sparse Float32 output, like FW_FZ_NZ).
namespace {

template <typename V> struct CscPay;
template <> struct CscPay<int32_t> {
    typedef unsigned long long T;
    __device__ static T make(int j, long long, int32_t v, uint32_t *) { return ((unsigned long long)(uint32_t)j << 32) | (uint32_t)v; }
    __device__ static int col(T w, const uint32_t *) { return (int)(w >> 32); }
    __device__ static int32_t val(T w, const int32_t *) { return (int32_t)(uint32_t)w; }
    __device__ static int bad(int32_t v) { return v > 0 ? 0 : v == 0 ? FW_CSC_ZERO : FW_CSC_NEGATIVE; }
};
template <> struct CscPay<double> {
    typedef uint32_t T;
    __device__ static T make(int j, long long e, double, uint32_t *ecol)
    {
        ecol[e] = (uint32_t)j;
        return (uint32_t)e;
    }
    __device__ static int col(T w, const uint32_t *ecol) { return (int)ecol[w]; }
    __device__ static double val(T w, const double *nzval) { return nzval[w]; }
    __device__ static int bad(double v)  // (-0.0 == 0: a stored zero; NaN fails every comparison)
    {
        return (v > 0.0 && v <= 1.7976931348623157e308) ? 0 : v == 0.0 ? FW_CSC_ZERO : v < 0.0 && v >= -1.7976931348623157e308 ? FW_CSC_NEGATIVE : FW_CSC_NONFINITE;
    }
};

// colstat[j]: 1 kept, 0 constant (dropped), < 0: -(FW_CSC_* flags).  pay[e] = the entry's payload for the sort by row (CscPay).
template <typename V>
__global__ __launch_bounds__(256) void csc_col_scan_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowval,
                                                           const V *__restrict__ nzval, int n, int p, long long nnz,
                                                           int32_t *__restrict__ colstat, typename CscPay<V>::T *__restrict__ pay,
                                                           uint32_t *__restrict__ ecol)
{
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= p) return;
    long long a, b;
    int bad = fw_csc_check_column(colptr, rowval, j, n, nnz, lane, &a, &b);
    V lo = NormVal<V>::vmax(), hi = NormVal<V>::vmin();
    for (long long e = a + lane; e < b; e += 64) {
        const V v = nzval[e];
        bad |= CscPay<V>::bad(v);
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        pay[e] = CscPay<V>::make(j, e, v, ecol);
    }
    bad = fw_wave_or(bad);
    for (int o = 32; o > 0; o >>= 1) {
        const V l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    if (lane == 0) {
        const long long cnt = b - a;  // (cnt < n: the implicit zeros differ from the stored values > 0)
        colstat[j] = bad ? -bad : (cnt == 0 || (cnt == (long long)n && lo == hi)) ? 0 : 1;
    }
}

// one thread per row over its run of the row-sorted entries: the totals of norm_row_stats_kernel + the host's chunk reduction
template <typename V>
__global__ __launch_bounds__(256) void csc_row_stats_kernel(const uint32_t *__restrict__ krow, const typename CscPay<V>::T *__restrict__ pay,
                                                            const V *__restrict__ nzval, const uint32_t *__restrict__ ecol,
                                                            long long nnz, int n, const int32_t *__restrict__ colq, int pk,
                                                            double *__restrict__ S, double *__restrict__ SL, int32_t *__restrict__ CNT,
                                                            V *__restrict__ MN, float *__restrict__ S32)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    long long lo = 0, hi = nnz;  // first entry of row i
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (krow[mid] < (uint32_t)i)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int per = (pk + NORM_CHUNKS - 1) / NORM_CHUNKS;
    double s = 0.0, sl = 0.0, cs = 0.0, csl = 0.0;
    float s32 = 0.0f;  // TSS: norm_row_tss_kernel's sum -- the run holds the row's stored terms in ascending column order
    int cc = 0, cnt = 0;
    V mn = NormVal<V>::vmax();
    for (long long e = lo; e < nnz && krow[e] == (uint32_t)i; ++e) {
        const typename CscPay<V>::T w = pay[e];
        const int q = colq[CscPay<V>::col(w, ecol)];
        if (q < 0) continue;
        const V v = CscPay<V>::val(w, nzval);
        const int c = q / per;
        if (c != cc) {  // chunk boundary of the dense kernel: its partial joins the total, the next starts from 0.0
            s += cs;
            sl += csl;
            cs = csl = 0.0;
            cc = c;
        }
        cs += (double)v;
        csl += log((double)v);
        s32 += (float)v;
        ++cnt;
        mn = v < mn ? v : mn;
    }
    S[i] = s + cs;
    SL[i] = sl + csl;
    CNT[i] = cnt;
    MN[i] = mn;
    if (S32) S32[i] = s32;
}

// binned_nz_clr, one workgroup per kept column: norm_binned_kernel with the keys read from the column's stored run (every entry
// of a kept column lies in a kept row: its count >= 1 gives the row reads).  bins[e] for the input entry e; M = the padded
// length of the longest kept column (sizes the key storage), each column sorts its own power of two.  One kernel for both
// launch shapes (256 threads while M <= 2 048, the HE case; 1 024 beyond): the bound of 1 024 caps it at 128 VGPRs, it uses 74 at most (with
// options 93: the registers of nb_compact's runs), so the short form loses no occupancy to the cap.
template <typename V, bool TSS, bool OPTS>
__global__ __launch_bounds__(1024) void csc_binned_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowval,
                                                          const V *__restrict__ nzval, const int32_t *__restrict__ cols, int pk,
                                                          const int32_t *__restrict__ rownew, const double *__restrict__ gmean,
                                                          const float *__restrict__ rsum32, int32_t *__restrict__ bins,
                                                          int32_t *__restrict__ two, int M, double *gkeys, int nb, int rank_dense,
                                                          int disc_mean)
{
    extern __shared__ double s_key_lds[];
    __shared__ int s_part[16];
    __shared__ unsigned long long s_wmask[16];
    const int tid = threadIdx.x, nt = blockDim.x;
    const NbKeys K{gkeys ? gkeys + (size_t)blockIdx.x * (size_t)M : s_key_lds, gkeys != nullptr};
    for (int q = blockIdx.x; q < pk; q += gridDim.x) {
        const long long a = colptr[cols[q]];
        const int m = (int)(colptr[cols[q] + 1] - a);
        int Mq = 2;
        while (Mq < m) Mq <<= 1;
        __syncthreads();  // (the previous column's last readers of the keys / s_wmask)
        for (int k = tid; k < m; k += nt) K.st(k, nb_key<TSS>(nzval[a + k], gmean, rownew[rowval[a + k]], rsum32, rowval[a + k]));
        K.sync();
        nb_pad_sort(K, m, Mq, tid, nt);
        const NbRule R = nb_rule<OPTS>(K, m, nb, rank_dense, disc_mean, tid, nt, s_part);
        unsigned long long seen = 0;
        for (int k = tid; k < m; k += nt) {
            const int bin = nb_bin(K, R, nb_key<TSS>(nzval[a + k], gmean, rownew[rowval[a + k]], rsum32, rowval[a + k]));
            seen |= 1ull << bin;
            bins[a + k] = bin;
        }
        const bool all = nb_all_levels(seen, nb, tid, nt, s_wmask);
        if (tid == 0) two[q] = all;
    }
}

// one wavefront per output column f = input column fcols[f]: rows renumbered, values by mode
//   0 FW_MI: 1    1 FW_MI_NZ / FW_NORM_TSS_BINNED: bins[e]    2 FW_FZ_NZ: (float)log(x / g_row), as norm_clr_out_kernel's mode 1
//   3 FW_NORM_TSS: (float)x / rsum32[input row], as norm_tss_out_kernel; a quotient that underflows to 0.0f stays a stored entry
template <typename V>
__global__ __launch_bounds__(256) void csc_emit_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowval,
                                                       const V *__restrict__ nzval, const int32_t *__restrict__ fcols, int pf,
                                                       const int64_t *__restrict__ ocolptr, const int32_t *__restrict__ rownew,
                                                       const double *__restrict__ gmean, const float *__restrict__ rsum32,
                                                       const int32_t *__restrict__ bins, int mode,
                                                       int32_t *__restrict__ orow, int32_t *__restrict__ oi, float *__restrict__ of)
{
    const int lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= pf) return;
    const long long a = colptr[fcols[f]], dst = ocolptr[f];
    const int m = (int)(ocolptr[f + 1] - dst);
    for (int k = lane; k < m; k += 64) {
        const int r = rownew[rowval[a + k]];
        orow[dst + k] = r;
        if (mode == 0)
            oi[dst + k] = 1;
        else if (mode == 1)
            oi[dst + k] = bins[a + k];
        else if (mode == 2)
            of[dst + k] = (float)log((double)nzval[a + k] / gmean[r]);
        else
            of[dst + k] = (float)nzval[a + k] / rsum32[rowval[a + k]];
    }
}

// FW_FZ (clr_adapt), dense nk x pk output: every cell as an absent one (norm_clr_out_kernel's mode 0 with x == 0) ...
__global__ __launch_bounds__(256) void csc_adapt_fill_kernel(int nk, int pk, const double *__restrict__ pseudo, const double *__restrict__ gmean,
                                                             float *__restrict__ out)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= nk) return;
    const float o = (float)log(pseudo[r] / gmean[r]);
    for (int q = blockIdx.y; q < pk; q += gridDim.y) out[(size_t)q * nk + r] = o;
}

// ... then the stored entries of the kept columns over them, one wavefront per kept column (entries of dropped rows are skipped)
template <typename V>
__global__ __launch_bounds__(256) void csc_adapt_scatter_kernel(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowval,
                                                                const V *__restrict__ nzval, const int32_t *__restrict__ cols, int pk,
                                                                const int32_t *__restrict__ rownew, int nk, const double *__restrict__ gmean,
                                                                float *__restrict__ out)
{
    const int lane = threadIdx.x & 63, q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= pk) return;
    const long long a = colptr[cols[q]], b = colptr[cols[q] + 1];
    for (long long e = a + lane; e < b; e += 64) {
        const int r = rownew[rowval[e]];
        if (r >= 0) out[(size_t)q * nk + r] = (float)log((double)nzval[e] / gmean[r]);
    }
}

// The input triple on the device and, per entry, its payload for the sort by row (Float64: the entry's index, its column in ecol).
// cp / rv / nz are what the kernels read: the uploaded copies (stage) or, in the *_csc_dev forms, the caller's own device arrays (borrow).
template <typename V> struct CscDev {
    FwDevArray<int64_t> colptr;
    FwDevArray<int32_t> rowval;
    FwDevArray<V> nzval;
    const int64_t *cp = nullptr;
    const int32_t *rv = nullptr;
    const V *nz = nullptr;
    FwDevArray<typename CscPay<V>::T> pay;
    FwDevArray<uint32_t> ecol;
    hipError_t stage(const int64_t *h_colptr, const int32_t *h_rowval, const V *h_nzval, int p, long long nnz)
    {
        hipError_t e = colptr.upload(h_colptr, (size_t)p + 1);
        if (e == hipSuccess) e = rowval.upload(h_rowval, (size_t)nnz);
        if (e == hipSuccess) e = nzval.upload(h_nzval, (size_t)nnz);
        cp = colptr.get(), rv = rowval.get(), nz = nzval.get();
        return e;
    }
    void borrow(const int64_t *d_colptr, const int32_t *d_rowval, const V *d_nzval) { cp = d_colptr, rv = d_rowval, nz = d_nzval; }
};

// The CSC filters.  Columns: structure and value check, var(data, dims=1) .> 0 (colq: input column -> its place in cols, or -1).  Row
// totals: the CSR view (a stable sort of the entries by row; the payload: CscPay), then one thread per row over its run.
// D holds the triple already, staged or borrowed.
template <typename V> int csc_filters(NormCall &c, int p, long long nnz, CscDev<V> &D)
{
    typedef typename CscPay<V>::T Pay;
    const int n = c.n;
    FwDevArray<int32_t> d_colstat, d_colq, d_cnt;
    FwDevArray<uint32_t> d_krow;
    FwDevArray<Pay> d_pay2;
    FwDevArray<char> d_tmp;
    FwDevArray<double> d_S, d_SL;
    FwDevArray<V> d_mn;
    std::vector<int32_t> colstat((size_t)p), colq((size_t)p, -1), CNT((size_t)n);
    std::vector<V> MN((size_t)n);
    std::vector<float> s32(c.K.tss ? (size_t)n : 0);
    NormTotals T{std::vector<double>((size_t)n), std::vector<double>((size_t)n), std::vector<double>((size_t)n), std::vector<int64_t>((size_t)n)};
    FW_HIP(nullptr, d_colstat.alloc((size_t)p));
    FW_HIP(nullptr, D.pay.alloc((size_t)nnz));
    if (sizeof(Pay) == sizeof(uint32_t)) FW_HIP(nullptr, D.ecol.alloc((size_t)nnz));  // (Float64: the payload is the entry's index)
    hipLaunchKernelGGL(csc_col_scan_kernel<V>, dim3((unsigned)((p + 3) / 4)), dim3(256), 0, 0, D.cp, D.rv, D.nz, n, p, nnz, d_colstat.get(), D.pay.get(), D.ecol.get());
    FW_HIP(nullptr, hipGetLastError());
    FW_HIP(nullptr, d_colstat.download(colstat));
    for (int j = 0; j < p; ++j) {
        if (colstat[j] < 0) return fw_fail(nullptr, FW_ERR_ARG, "%s: column %d: %s", c.fn, j, fw_csc_reason(-colstat[j]));
        c.col_mask[j] = colstat[j] != 0;  // var(data, dims=1) .> 0
        if (c.col_mask[j]) {
            colq[j] = (int32_t)c.cols.size();
            c.cols.push_back(j);
        }
    }
    const int pk = (int)c.cols.size();
    if (pk == 0) return norm_all_constant(c.fn);
    int bits = 1;
    while ((1ll << bits) < (long long)n) ++bits;
    size_t tb = 0;
    FW_HIP(nullptr, d_krow.alloc((size_t)nnz));
    FW_HIP(nullptr, d_pay2.alloc((size_t)nnz));
    FW_HIP(nullptr, (rocprim::radix_sort_pairs(nullptr, tb, (const uint32_t *)D.rv, d_krow.get(), (const Pay *)D.pay.get(), d_pay2.get(), (size_t)nnz, 0u, (unsigned int)bits, (hipStream_t)0)));
    FW_HIP(nullptr, d_tmp.alloc(tb ? tb : 1));
    FW_HIP(nullptr, (rocprim::radix_sort_pairs((void *)d_tmp.get(), tb, (const uint32_t *)D.rv, d_krow.get(), (const Pay *)D.pay.get(), d_pay2.get(), (size_t)nnz, 0u, (unsigned int)bits, (hipStream_t)0)));
    FW_HIP(nullptr, d_colq.upload(colq));
    FW_HIP(nullptr, d_S.alloc((size_t)n));
    FW_HIP(nullptr, d_SL.alloc((size_t)n));
    FW_HIP(nullptr, d_cnt.alloc((size_t)n));
    FW_HIP(nullptr, d_mn.alloc((size_t)n));
    if (c.K.tss) FW_HIP(nullptr, c.d_s32.alloc((size_t)n));
    hipLaunchKernelGGL(csc_row_stats_kernel<V>, dim3((n + 255) / 256), dim3(256), 0, 0, d_krow.get(), d_pay2.get(), D.nz, D.ecol.get(), nnz, n, d_colq.get(),
                       pk, d_S.get(), d_SL.get(), d_cnt.get(), d_mn.get(), c.d_s32.get());
    FW_HIP(nullptr, hipGetLastError());
    FW_HIP(nullptr, d_S.download(T.S));
    FW_HIP(nullptr, d_SL.download(T.SL));
    FW_HIP(nullptr, d_cnt.download(CNT));
    FW_HIP(nullptr, d_mn.download(MN));
    if (c.K.tss) FW_HIP(nullptr, c.d_s32.download(s32));
    for (int i = 0; i < n; ++i) {
        T.NZ[i] = (int64_t)pk - CNT[i];
        T.RMIN[i] = (double)MN[i];
    }
    return norm_rows(c, NormVal<V>::tie_rel(pk), T, s32);
}

// CSC output.  FW_FZ (clr_adapt): the dense matrix, pseudo-count cells first, the stored entries over them.  The sparse kinds: the
// kind's own column filter, then the output triple (every entry of a kept column lies in a kept row: a column keeps its length).
// The outputs are host buffers the result is downloaded into, or (c.dev_out) device buffers of the caller that the kernels write.
template <typename V> int csc_output(NormCall &c, long long nnz, const int64_t *colptr, const CscDev<V> &D, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32, int64_t *nnz_out)
{
    const int nk = (int)c.R.rows.size(), pk = (int)c.cols.size();
    FwDevArray<int32_t> d_rownew, d_bins, d_two, d_orow, d_oi;
    FwDevArray<int64_t> d_ocolptr;
    FwDevArray<double> d_g, d_pseudo;
    FwDevArray<float> d_of;
    std::vector<int32_t> two(c.K.binned ? (size_t)pk : 0);
    if (nk == 0) return norm_none_left(c);  // (FW_FZ alone drops samples with reads)
    FW_HIP(nullptr, d_rownew.upload(norm_rownew(c.n, c.R.rows)));
    FW_HIP(nullptr, c.d_cols.upload(c.cols));
    FW_HIP(nullptr, d_g.upload(c.R.g));
    if (c.kind == FW_FZ) {
        FW_HIP(nullptr, d_pseudo.upload(c.R.pseudo));
        if (!c.dev_out) FW_HIP(nullptr, d_of.alloc((size_t)nk * pk));
        float *of = c.dev_out ? out_f32 : d_of.get();
        hipLaunchKernelGGL(csc_adapt_fill_kernel, norm_out_grid(nk, pk), dim3(256), 0, 0, nk, pk, d_pseudo.get(), d_g.get(), of);
        hipLaunchKernelGGL(csc_adapt_scatter_kernel<V>, dim3((unsigned)((pk + 3) / 4)), dim3(256), 0, 0, D.cp, D.rv, D.nz, c.d_cols.get(), pk, d_rownew.get(), nk, d_g.get(), of);
        FW_HIP(nullptr, hipGetLastError());
        if (c.dev_out) FW_HIP(nullptr, hipStreamSynchronize(0));  // (the caller reads its buffer at once)
        if (!c.dev_out) FW_HIP(nullptr, d_of.download(out_f32, (size_t)nk * pk));
        *nnz_out = (int64_t)nk * pk;
        return FW_OK;
    }
    if (c.K.binned) {
        const auto binned = c.O.plain() ? (!c.K.tss ? csc_binned_kernel<V, false, false> : csc_binned_kernel<V, true, false>)  // (the key: nb_key)
                                        : (!c.K.tss ? csc_binned_kernel<V, false, true> : csc_binned_kernel<V, true, true>);
        int64_t mmax = 0;
        for (int j : c.cols) mmax = std::max(mmax, colptr[j + 1] - colptr[j]);
        NormBinShape B;
        if (int rc = norm_bin_shape((const void *)binned, mmax, pk, false, B)) return rc;
        FW_HIP(nullptr, d_bins.alloc((size_t)nnz));
        FW_HIP(nullptr, d_two.alloc((size_t)pk));
        hipLaunchKernelGGL(binned, dim3(B.grid), dim3(B.threads), B.lds(), 0, D.cp, D.rv, D.nz, c.d_cols.get(), pk, d_rownew.get(),
                           d_g.get(), c.d_s32.get(), d_bins.get(), d_two.get(), B.M, B.keys.get(), c.O.b, (int)c.O.dense, (int)c.O.mean);
        FW_HIP(nullptr, hipGetLastError());
        FW_HIP(nullptr, d_two.download(two));
    } else if (c.K.none_left) {  // FW_MI, presabs_norm!: two levels among the kept samples <=> an absence among them
        for (int j : c.cols) two.push_back(colptr[j + 1] - colptr[j] < (int64_t)nk);
    }
    if (!two.empty() && norm_keep_columns(two, c.cols, c.col_mask).empty()) return norm_none_left(c);
    const int pf = (int)c.cols.size();
    const std::vector<int64_t> ocolptr = norm_out_colptr(colptr, c.cols);
    const size_t onnz = (size_t)ocolptr[pf];
    FW_HIP(nullptr, hipMemcpy(c.d_cols.get(), c.cols.data(), sizeof(int32_t) * (size_t)pf, hipMemcpyHostToDevice));
    if (c.dev_out) {  // the caller's device buffers take the output triple where the kernel writes it (onnz <= nnz, pf <= p)
        FW_HIP(nullptr, hipMemcpy(out_colptr, ocolptr.data(), sizeof(int64_t) * ((size_t)pf + 1), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(csc_emit_kernel<V>, dim3((unsigned)((pf + 3) / 4)), dim3(256), 0, 0, D.cp, D.rv, D.nz, c.d_cols.get(), pf,
                           (const int64_t *)out_colptr, d_rownew.get(), d_g.get(), c.d_s32.get(), d_bins.get(), c.K.emit_mode, out_rowval, c.K.i32 ? out_i32 : nullptr,
                           c.K.i32 ? nullptr : out_f32);
        FW_HIP(nullptr, hipGetLastError());
        FW_HIP(nullptr, hipStreamSynchronize(0));
        *nnz_out = (int64_t)onnz;
        return FW_OK;
    }
    FW_HIP(nullptr, d_ocolptr.upload(ocolptr));
    FW_HIP(nullptr, d_orow.alloc(onnz));
    if (c.K.i32) FW_HIP(nullptr, d_oi.alloc(onnz));
    if (!c.K.i32) FW_HIP(nullptr, d_of.alloc(onnz));
    hipLaunchKernelGGL(csc_emit_kernel<V>, dim3((unsigned)((pf + 3) / 4)), dim3(256), 0, 0, D.cp, D.rv, D.nz, c.d_cols.get(), pf,
                       d_ocolptr.get(), d_rownew.get(), d_g.get(), c.d_s32.get(), d_bins.get(), c.K.emit_mode, d_orow.get(), d_oi.get(), d_of.get());
    FW_HIP(nullptr, hipGetLastError());
    FW_HIP(nullptr, d_orow.download(out_rowval, onnz));
    if (c.K.i32) FW_HIP(nullptr, d_oi.download(out_i32, onnz));
    if (!c.K.i32) FW_HIP(nullptr, d_of.download(out_f32, onnz));
    std::copy(ocolptr.begin(), ocolptr.end(), out_colptr);
    *nnz_out = (int64_t)onnz;
    return FW_OK;
}

// The CSC front-end for either value type (fn: the entry point's name, for the messages).
template <typename V>
int norm_csc(const char *fn, int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval, const V *nzval,
             int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
             const fw_norm_opts *opts)
{
    if (!colptr || !row_mask || !col_mask || !n_out || !p_out || !nnz_out || n <= 0 || p <= 0) return fw_fail(nullptr, FW_ERR_ARG, "%s: invalid argument", fn);
    NormCall c{fn, kind, norm_kind(kind), n, row_mask, col_mask};
    if (int rc = norm_call_check(c, opts)) return rc;
    if ((c.K.i32 ? !out_i32 : !out_f32) || (kind != FW_FZ && (!out_colptr || !out_rowval))) return fw_fail(nullptr, FW_ERR_ARG, "%s: missing output buffer", fn);
    const long long nnz = colptr[p];
    if (colptr[0] != 0 || nnz < 0) return fw_fail(nullptr, FW_ERR_ARG, "%s: colptr must run from 0 to nnz (column 0)", fn);
    if (nnz > 0x7fffffffll) return fw_fail(nullptr, FW_ERR_LIMIT, "%s: %lld stored entries exceed the 32-bit entry index", fn, nnz);
    if (nnz > 0 && (!rowval || !nzval)) return fw_fail(nullptr, FW_ERR_ARG, "%s: NULL array", fn);
    if (nnz == 0) return norm_all_constant(fn);
    CscDev<V> D;
    FW_HIP(nullptr, hipSetDevice(device));
    FW_HIP(nullptr, D.stage(colptr, rowval, nzval, p, nnz));
    if (int rc = csc_filters(c, p, nnz, D)) return rc;
    if (int rc = csc_output(c, nnz, colptr, D, out_colptr, out_rowval, out_i32, out_f32, nnz_out)) return rc;
    *n_out = (int32_t)c.R.rows.size();
    *p_out = (int32_t)c.cols.size();
    return FW_OK;
}

// The *_csc_dev forms: the triple and the output buffers in device memory of `device` (include/flashweave_amd.h).  Every pointer is
// asked of the runtime first; then the p + 1 column pointers are downloaded and must run monotonically from 0 to nnz before any kernel
// reads rowval or nzval (the kernels' own column check stays).  The triple is borrowed, the output written in place; the stages and
// their kernels are those of norm_csc, so the bits are.
template <typename V>
int norm_csc_dev(const char *fn, int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *d_colptr, const int32_t *d_rowval, const V *d_nzval,
                 int64_t nnz, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out,
                 int32_t *p_out, int64_t *nnz_out, const fw_norm_opts *opts)
{
    if (!row_mask || !col_mask || !n_out || !p_out || !nnz_out || n <= 0 || p <= 0) return fw_fail(nullptr, FW_ERR_ARG, "%s: invalid argument", fn);
    NormCall c{fn, kind, norm_kind(kind), n, row_mask, col_mask};
    if (int rc = norm_call_check(c, opts)) return rc;
    c.dev_out = true;
    if (int rc = fwi_csc_dev_ptrs(nullptr, fn, device, d_colptr, d_rowval, d_nzval, nnz)) return rc;
    const void *value_out = c.K.i32 ? (const void *)out_i32 : (const void *)out_f32;
    if (!value_out || (kind != FW_FZ && (!out_colptr || !out_rowval))) return fw_fail(nullptr, FW_ERR_ARG, "%s: missing output buffer", fn);
    if (!fw_is_dev_ptr(value_out, device) || (kind != FW_FZ && (!fw_is_dev_ptr(out_colptr, device) || !fw_is_dev_ptr(out_rowval, device))))
        return fw_fail(nullptr, FW_ERR_ARG, "%s: the output buffer is not device memory of device %d", fn, device);
    if (nnz > 0x7fffffffll) return fw_fail(nullptr, FW_ERR_LIMIT, "%s: %lld stored entries exceed the 32-bit entry index", fn, (long long)nnz);
    FW_HIP(nullptr, hipSetDevice(device));
    std::vector<int64_t> colptr;
    if (int rc = fwi_csc_dev_colptr(nullptr, fn, d_colptr, p, nnz, colptr)) return rc;
    if (nnz == 0) return norm_all_constant(fn);
    CscDev<V> D;
    D.borrow(d_colptr, d_rowval, d_nzval);
    if (int rc = csc_filters(c, p, nnz, D)) return rc;
    if (int rc = csc_output(c, nnz, colptr.data(), D, out_colptr, out_rowval, out_i32, out_f32, nnz_out)) return rc;
    *n_out = (int32_t)c.R.rows.size();
    *p_out = (int32_t)c.cols.size();
    return FW_OK;
}

}  // namespace

extern "C" int fw_normalize_counts_csc_opts(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval,
                                            const int32_t *nzval, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32,
                                            uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
                                            const fw_norm_opts *opts)
{
    return norm_csc<int32_t>(opts ? "fw_normalize_counts_csc_opts" : "fw_normalize_counts_csc", device, kind, n, p, colptr, rowval, nzval, out_colptr, out_rowval, out_i32,
                             out_f32, row_mask, col_mask, n_out, p_out, nnz_out, opts);
}

extern "C" int fw_normalize_counts_csc(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval,
                                       const int32_t *nzval, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32,
                                       uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out)
{
    return fw_normalize_counts_csc_opts(device, kind, n, p, colptr, rowval, nzval, out_colptr, out_rowval, out_i32, out_f32, row_mask, col_mask, n_out, p_out, nnz_out, nullptr);
}

extern "C" int fw_normalize_abund_csc_opts(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval,
                                           const double *nzval, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32,
                                           uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
                                           const fw_norm_opts *opts)
{
    return norm_csc<double>(opts ? "fw_normalize_abund_csc_opts" : "fw_normalize_abund_csc", device, kind, n, p, colptr, rowval, nzval, out_colptr, out_rowval, out_i32,
                            out_f32, row_mask, col_mask, n_out, p_out, nnz_out, opts);
}

extern "C" int fw_normalize_abund_csc(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *colptr, const int32_t *rowval,
                                      const double *nzval, int64_t *out_colptr, int32_t *out_rowval, int32_t *out_i32, float *out_f32,
                                      uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out)
{
    return fw_normalize_abund_csc_opts(device, kind, n, p, colptr, rowval, nzval, out_colptr, out_rowval, out_i32, out_f32, row_mask, col_mask, n_out, p_out, nnz_out, nullptr);
}

// The *_csc_dev forms: the triple and the output buffers in device memory (include/flashweave_amd.h); opts == NULL means the defaults.
extern "C" int fw_normalize_counts_csc_dev(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *d_colptr, const int32_t *d_rowval,
                                           const int32_t *d_nzval, int64_t nnz, int64_t *d_out_colptr, int32_t *d_out_rowval, int32_t *d_out_i32,
                                           float *d_out_f32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
                                           const fw_norm_opts *opts)
{
    return norm_csc_dev<int32_t>("fw_normalize_counts_csc_dev", device, kind, n, p, d_colptr, d_rowval, d_nzval, nnz, d_out_colptr, d_out_rowval, d_out_i32, d_out_f32,
                                 row_mask, col_mask, n_out, p_out, nnz_out, opts);
}

extern "C" int fw_normalize_abund_csc_dev(int32_t device, int32_t kind, int32_t n, int32_t p, const int64_t *d_colptr, const int32_t *d_rowval,
                                          const double *d_nzval, int64_t nnz, int64_t *d_out_colptr, int32_t *d_out_rowval, int32_t *d_out_i32,
                                          float *d_out_f32, uint8_t *row_mask, uint8_t *col_mask, int32_t *n_out, int32_t *p_out, int64_t *nnz_out,
                                          const fw_norm_opts *opts)
{
    return norm_csc_dev<double>("fw_normalize_abund_csc_dev", device, kind, n, p, d_colptr, d_rowval, d_nzval, nnz, d_out_colptr, d_out_rowval, d_out_i32, d_out_f32,
                                row_mask, col_mask, n_out, p_out, nnz_out, opts);
}
