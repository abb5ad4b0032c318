// The host rules of the normalisation front-end (fw_norm.hip) -- which samples and columns survive, with which parameters: plain C++17
// over vectors, no HIP and no fw_internal.h, so that tests/native/norm_host_check.cpp compiles it with g++ alone (tests/test_norm_host_cpu.py).
// The dense and the CSC driver both come here: the same libm calls on the same bits.  A refusal is a value; fw_norm.hip words the message.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/flashweave_amd.h"

#define NORM_CHUNKS 64  // column chunks of norm_row_stats_kernel: the order of the additions, so part of the result
enum { NORM_CLR_ADAPT = 0, NORM_CLR_NZ = 1 };                                         // norm_clr_out_kernel's mode
enum { CSC_EMIT_ONE = 0, CSC_EMIT_BINS = 1, CSC_EMIT_CLR_NZ = 2, CSC_EMIT_TSS = 3 };  // csc_emit_kernel's mode

// What a `kind` means to the drivers, decoded once per call.  known: one of the six; i32: Int32 output (out_i32), else Float32
// (out_f32); tss: needs the Float32 row sums; binned: the rank / bin kernels, with the TSS quotient as the key when tss; the mode of
// norm_clr_out_kernel (the two clr kinds) and of csc_emit_kernel (every kind but FW_FZ, whose CSC form is dense); none_left: the
// refusal when the kind's own filter leaves nothing (nullptr: it has none).
struct NormKind {
    bool known, i32, tss, binned;
    int clr_mode, emit_mode;
    const char *none_left;
};

inline NormKind norm_kind(int kind)
{
    static const char *no_bins = "no column whose non-zero abundances fall into two bins";
    switch (kind) {
    case FW_FZ: return {true, false, false, false, NORM_CLR_ADAPT, -1, "no sample is left after the pseudo-counts"};
    case FW_FZ_NZ: return {true, false, false, false, NORM_CLR_NZ, CSC_EMIT_CLR_NZ, nullptr};
    case FW_MI: return {true, true, false, false, -1, CSC_EMIT_ONE, "no column with two levels"};
    case FW_MI_NZ: return {true, true, false, true, -1, CSC_EMIT_BINS, no_bins};
    case FW_NORM_TSS: return {true, false, true, false, -1, CSC_EMIT_TSS, nullptr};
    case FW_NORM_TSS_BINNED: return {true, true, true, true, -1, CSC_EMIT_BINS, no_bins};
    }
    return {false, false, false, false, -1, -1, nullptr};
}

// The options of the binned kinds (fw_norm_opts) as the kernels take them: b = n_bins - 1 non-zero bins, the dense instead of the tied
// rank, the "mean" instead of the "median" rule.  The defaults are what the front-end computed before it had options.
#define NORM_BINS_MAX 62  // n_bins - 1 <= 61: the levels 1 .. b are the bits of one 64-bit mask, and the engine takes at most 62 levels
struct NormOpts {
    int b = 2;
    bool dense = false, mean = false;
    bool plain() const { return b == 2 && !dense && !mean; }  // the defaults: the kernels' instantiation without options
};

// fw_norm_opts (nullptr: the defaults) against the kind -> nullptr and `out`, or the refusal in words that name the field.
inline const char *norm_opts_check(const fw_norm_opts *o, const NormKind &K, NormOpts &out)
{
    out = NormOpts();
    if (!o) return nullptr;
    if (o->n_bins < 3 || o->n_bins > NORM_BINS_MAX) return "n_bins must lie in 3 .. 62 (two levels are the kind FW_MI)";
    if (o->rank_method != FW_RANK_TIED && o->rank_method != FW_RANK_DENSE) return "rank_method must be FW_RANK_TIED or FW_RANK_DENSE";
    if (o->disc_method != FW_DISC_MEDIAN && o->disc_method != FW_DISC_MEAN) return "disc_method must be FW_DISC_MEDIAN or FW_DISC_MEAN";
    if (o->disc_method == FW_DISC_MEAN && o->n_bins > 3) return "disc_method FW_DISC_MEAN only works with 2 non-zero bins (n_bins = 3)";
    if (!K.binned) {
        if (o->n_bins != 3) return "n_bins applies to the binned kinds only (FW_MI_NZ, FW_NORM_TSS_BINNED)";
        if (o->rank_method != FW_RANK_TIED) return "rank_method applies to the binned kinds only (FW_MI_NZ, FW_NORM_TSS_BINNED)";
        if (o->disc_method != FW_DISC_MEDIAN) return "disc_method applies to the binned kinds only (FW_MI_NZ, FW_NORM_TSS_BINNED)";
    }
    out.b = o->n_bins - 1;
    out.dense = o->rank_method == FW_RANK_DENSE;
    out.mean = o->disc_method == FW_DISC_MEAN;
    return nullptr;
}

// A refusal as a value (reason == nullptr: none).  sample >= 0: the Float32 sum of that sample is `reason` ("zero" / "infinite").
struct NormRefusal {
    const char *reason = nullptr;
    int sample = -1;
};

// Per-row totals over the kept columns (n values each): S read sum, SL sum of log over the non-zeros, NZ number of zeros, RMIN
// smallest non-zero (as Float64, exact for either value type).  NormRows: the kept samples (ascending input rows) and, per kept
// sample, the pseudo-count (FW_FZ) and the geometric mean (the clr kinds and FW_MI_NZ; 1 otherwise).
struct NormTotals {
    std::vector<double> S, SL, RMIN;
    std::vector<int64_t> NZ;
};
struct NormRows {
    std::vector<int32_t> rows;
    std::vector<double> pseudo, g;
};

// the NORM_CHUNKS partials of norm_row_stats_kernel ([chunk][row]) -> totals, added in chunk order from 0.0 (deterministic)
template <typename V> NormTotals norm_reduce_chunks(int n, const std::vector<double> &rsum, const std::vector<double> &rlog, const std::vector<int32_t> &rzero, const std::vector<V> &rmin)
{
    const std::vector<double> zero((size_t)n, 0.0);
    NormTotals T{zero, zero, std::vector<double>((size_t)n, INFINITY), std::vector<int64_t>((size_t)n, 0)};
    for (int c = 0; c < NORM_CHUNKS; ++c)
        for (int i = 0; i < n; ++i) {
            const size_t k = (size_t)c * n + i;
            T.S[i] += rsum[k];
            T.SL[i] += rlog[k];
            T.NZ[i] += rzero[k];
            T.RMIN[i] = std::min(T.RMIN[i], (double)rmin[k]);
        }
    return T;
}

// Totals -> kept samples and their parameters; row_mask[n] is written.  rows = samples with reads; FW_FZ: adaptive pseudo-counts
// (a sample whose pseudo-count underflows to 0 is dropped) and the geometric mean of the filled row; FW_FZ_NZ / FW_MI_NZ: geometric
// mean of the non-zeros.  s32 (the TSS kinds, else nullptr): the Float32 sums of all n samples; those of the kept ones must be divisors,
// positive and finite.  A kept sample has a Float64 sum > 0; its Float32 sum is 0 only when every value vanishes as a Float32 (< 2^-150),
// and infinite only beyond the Float32 range: real-valued tables alone, which the Python front-ends refuse by name before any device call.
// tie_rel: the anchor of the pseudo-counts is the sample of maximal depth, and in a table of relative abundances every sample has
// the depth 1 up to the rounding of its sum, so the largest Float64 sum would be picked by the order of the additions (the dense
// and the CSC kernel, numpy and the reference each have their own).  Samples whose sums lie within tie_rel of the largest take part
// and the first of them is the anchor.  Real values: pk * 2^-52, the bound |fl(sum) - sum| <= (pk - 1) 2^-53 sum of any order of
// additions, on either side; not order-proof at the window's edge, see preprocess.adaptive_clr(tie_anchor=True), the host's form of
// the rule.  Counts: 0 -- their sums are exact -- which is the rule "first sample of maximal sum".
inline NormRefusal norm_row_params(int kind, int n, int pk, double tie_rel, const NormTotals &T, const std::vector<float> *s32, uint8_t *row_mask, NormRows &R)
{
    std::vector<int32_t> &rows = R.rows;
    rows.clear();
    double min_abund = INFINITY;
    for (int i = 0; i < n; ++i) {
        row_mask[i] = T.S[i] > 0.0;  // sum(data, dims=2) .> 0
        if (row_mask[i]) {
            rows.push_back(i);
            min_abund = std::min(min_abund, T.RMIN[i]);
        }
    }
    if (rows.empty()) return {"no sample has reads"};
    R.pseudo.assign(rows.size(), 0.0);
    R.g.assign(rows.size(), 1.0);
    if (kind == FW_FZ) {  // adaptive_pseudocount! (:157-190): row of maximal depth as the anchor
        double smax = 0.0;
        for (int i : rows) smax = std::max(smax, T.S[i]);
        int md = rows[0];
        for (int i : rows)
            if (T.S[i] >= smax * (1.0 - tie_rel)) {
                md = i;
                break;
            }
        const double base = min_abund >= 1.0 ? 1.0 : min_abund / 10.0;  // (counts: always 1; abundances below 1: a tenth of the smallest)
        const double k = (double)T.NZ[md], P = (double)pk, Nprod1 = T.SL[md];
        std::vector<int32_t> rows2;
        R.pseudo.clear();
        for (int i : rows) {
            const double nz = (double)T.NZ[i];
            if (!(nz < P && k < P)) return {"samples with all zero abundances are not allowed"};
            const double ps = std::exp((1.0 / (nz - P)) * ((k - P) * std::log(base) + Nprod1 - T.SL[i]));
            if (ps != 0.0) {
                rows2.push_back(i);
                R.pseudo.push_back(ps);
            } else {
                row_mask[i] = 0;
            }
        }
        rows.swap(rows2);
        R.g.resize(rows.size());
        for (size_t r = 0; r < rows.size(); ++r) {  // clr!(pseudo_count = 0): geometric mean of the filled row
            const int i = rows[r];
            R.g[r] = std::exp((T.SL[i] + (double)T.NZ[i] * std::log(R.pseudo[r])) / P);
        }
    } else if (kind == FW_FZ_NZ || kind == FW_MI_NZ) {  // geometric mean of the non-zeros
        for (size_t r = 0; r < rows.size(); ++r) {
            const int i = rows[r];
            const double cnt = (double)pk - (double)T.NZ[i];
            R.g[r] = cnt > 0 ? std::exp(T.SL[i] / cnt) : 1.0;
        }
    }
    if (s32)
        for (int i : rows)
            if (!((*s32)[i] > 0.0f && (*s32)[i] <= FLT_MAX)) return {(*s32)[i] > 0.0f ? "infinite" : "zero", i};
    return {};
}

// Keep the columns q with two[q] -> their places q (empty: none is left); cols (input ids, one per q) is compacted, a dropped column's mask bit cleared.
inline std::vector<int32_t> norm_keep_columns(const std::vector<int32_t> &two, std::vector<int32_t> &cols, uint8_t *col_mask)
{
    std::vector<int32_t> sel;
    for (size_t q = 0; q < cols.size(); ++q) {
        if (two[q]) sel.push_back((int32_t)q);
        if (!two[q]) col_mask[cols[q]] = 0;
    }
    for (size_t f = 0; f < sel.size(); ++f) cols[f] = cols[sel[f]];
    cols.resize(sel.size());
    return sel;
}

// row renumbering: the prefix sum over the row mask (-1: dropped)
inline std::vector<int32_t> norm_rownew(int n, const std::vector<int32_t> &rows)
{
    std::vector<int32_t> rownew((size_t)n, -1);
    for (size_t r = 0; r < rows.size(); ++r) rownew[rows[r]] = (int32_t)r;
    return rownew;
}

// column compaction: the scan over the stored lengths of the output columns fcols (input column ids)
inline std::vector<int64_t> norm_out_colptr(const int64_t *colptr, const std::vector<int32_t> &fcols)
{
    std::vector<int64_t> ocolptr(fcols.size() + 1, 0);
    for (size_t f = 0; f < fcols.size(); ++f) ocolptr[f + 1] = ocolptr[f] + (colptr[fcols[f] + 1] - colptr[fcols[f]]);
    return ocolptr;
}
