// The host job pool's plain records and pure rules (fw_pool.cpp): C++17 over plain values, no HIP and no fw_ctx, so that
// tests/native/pool_check.cpp can compile it with g++ alone (tests/test_pool_host_cpu.py).  Knob values arrive as arguments.
//
// A job's subsets are ranked in the reference's enumeration order (sizes max_k..1, lexicographic inside a size).  Ranks are evaluated
// in windows that grow geometrically; each window is cut into segments, one workgroup per segment, and the per-segment records are
// merged IN RANK ORDER: the first stopping rank ends the job exactly where the sequential reference would have stopped
// (tests.jl:326-336); otherwise the (p, rank) maximum with "later wins ties" is carried forward (tests.jl:338-341).  Speculation is
// bounded by the window growth factor.  tests/pool_plan.py restates the plan in Python; DhParams / dh_merge / mi_merge in
// fw_devhiton.hip are the device rounds' forms of the window policy and the merge.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/flashweave_amd.h"
#include "fw_unrank.h"

// ---- records (device layouts: the segment kernels read and write them) ----
// Job descriptor for the test_subsets kernels
struct FwJob {
    int32_t X;        // T
    int32_t Y;        // candidate
    int64_t acc_off;  // offset into the flat accepted array
    int32_t acc_len;  // |accepted|
    int32_t pad;
};

// Result of one job (mirrors fw_subsets_result without frac)
struct FwJobOut {
    double stat;
    double pval;
    int64_t num_tests;  // reference-equivalent count
    int64_t evaluated;  // tests evaluated by the kernel (speculation included)
    int32_t df;
    int32_t suff_power;
    int32_t status;
    int32_t n_zs;
    int32_t zs[FW_MAX_K];
    int32_t pad[3];
};

// One segment of a job: ranks [start, end) of the job's subset enumeration
struct FwSeg {
    int32_t X;
    int32_t Y;
    int64_t acc_off;
    int32_t acc_len;
    int32_t pad;
    uint64_t start;
    uint64_t end;
    // r06, fz device rounds: the target's LOCAL correlation matrix -- (tm_m x tm_m) Float32 over [T, its level-0 neighbours in ascending id
    // order], a copy of those entries of the p x p matrix (fw_devhiton.hip: dh_tmat_build_kernel) -- and the sorted ids; 0: none (host pool,
    // light targets): the kernel gathers from the p x p matrix
    uint64_t tm, tm_ids;
    int32_t tm_m, pad1;
};
static_assert(sizeof(FwSeg) == 64, "FwSeg is eight 64-bit words");

#define FW_RANK_NONE (~0ull)

// Result of one segment.  The conditioning sets are recovered on the host from the ranks.
struct FwSegOut {
    uint64_t stop_rank;  // first rank in the segment that ends the job (non-significant or max_tests), else FW_RANK_NONE
    double stop_stat;
    double stop_pval;
    uint64_t best_rank;  // last rank attaining the maximum p in the segment (valid when there was no stop)
    double best_stat;
    double best_pval;
    int32_t stop_df;     // -2 (fz_nz): too few rows with T != 0 and candidate != 0 -> no test at all
    int32_t stop_power;
    int32_t best_df;
    int32_t pad;
    uint64_t evaluated;
};
static_assert(sizeof(FwSegOut) == 72, "FwSegOut is nine 64-bit words");

// ---- enumeration ----
// C(m, t), saturating at 2^62: the shared forms of fw_unrank.h by their ranges (tests/test_pool_host_cpu.py holds them to a
// long-double restatement with the same bounds, on every m up to 65 536 and around each first saturating m)
inline uint64_t fw_pool_binom(int64_t m, int t) { return t <= 5 ? fw_binom_u64(m, t) : fw_binom_any(m, t); }

// ranks of a job with a accepted variables: sum of C(a, s) for s = max_k..1, saturating at 2^62, capped by max_tests (> 0)
inline uint64_t fw_pool_enum_size(int a, int max_k, int64_t max_tests)
{
    uint64_t N = 0;
    for (int s = max_k; s >= 1; --s) {
        N += fw_pool_binom(a, s);
        if (N > (1ull << 62)) N = 1ull << 62;
    }
    const uint64_t mt = max_tests > 0 ? (uint64_t)max_tests : 0;
    return (mt && mt < N) ? mt : N;
}

// lexicographic unranking (same order as the device code): rank -> subset size and positions in the accepted list
inline void fw_pool_unrank(uint64_t r, int a, int max_k, int *s_out, int *pos)
{
    int s = max_k;
    while (s > 1) {
        const uint64_t cnt = fw_pool_binom(a, s);
        if (r < cnt) break;
        r -= cnt;
        --s;
    }
    *s_out = s;
    int prev = -1;
    for (int d = 0; d < s; ++d) {
        const int t = s - d;
        int c = prev + 1;
        for (;;) {
            const uint64_t with_c = fw_pool_binom(a - 1 - c, t - 1);
            if (r < with_c) break;
            r -= with_c;
            ++c;
        }
        pos[d] = c;
        prev = c;
    }
}

// ---- window plan ----
// first window: fz 256 ranks (one test per lane of one workgroup), w0_big (16384) once |accepted| >= 64 -- a job that large either
// stops within the first few tests or runs for tens of thousands, so small first windows are wasted round trips (cfg3: 1731 -> 1154
// launches per pass, +4 % evaluated tests, 0.527 -> 0.50 s); discrete: 16
inline uint64_t fw_pool_first_window(bool fz_kind, int a, uint64_t w0_big) { return fz_kind ? (a >= 64 ? w0_big : 256ull) : 16ull; }

// ranks of the window [next, next + width) that exist
inline uint64_t fw_pool_window(uint64_t next, uint64_t width, uint64_t N) { return std::min(width, N - next); }

// segment length for a launch of `total` ranks: a few thousand workgroups.  fz: one lane per test (256-rank granularity, runs of up to
// 32 ranks per lane); discrete: one wavefront per test (4-rank granularity).  seg_target 0: the default (fz 3072, discrete 4096)
inline uint64_t fw_pool_seglen(uint64_t total, bool fz, uint64_t seg_target)
{
    const uint64_t q = fz ? 256 : 4, smin = fz ? 256 : 8, smax = fz ? 8192 : 256;
    const uint64_t seg_tgt = seg_target ? seg_target : (fz ? 3072 : 4096);
    const uint64_t seglen = (total / seg_tgt + q - 1) / q * q;
    return std::max<uint64_t>(smin, std::min<uint64_t>(seglen, smax));
}

inline uint64_t fw_pool_nsegs(uint64_t ranks, uint64_t seglen) { return (ranks + seglen - 1) / seglen; }

// the cut of the window [lo, hi) into segments of seglen ranks (the last one shorter): emit(start, end) in rank order
template <class Emit> inline void fw_pool_cut(uint64_t lo, uint64_t hi, uint64_t seglen, Emit &&emit)
{
    for (uint64_t s = lo; s < hi; s += seglen) emit(s, std::min(hi, s + seglen));
}

// geometric growth of the evaluation window of a job (speculation bound vs number of latency-bound rounds).  forced (2..64): that
// factor.  Many jobs in flight: launches are full, keep speculation tight (x4); few jobs: the round latency dominates and a wider
// window (x16) saves rounds (measured on cfg3: 3236 -> 2024 launches for +9 % evaluated tests); a launch that does not even fill the
// GPU (a few thousand workgroups of 256 ranks; small_launch, default 1 << 22 -- cfg3 sweep: 0 -> 630 ms, 1M 613, 4M 569, 8M 588,
// 64M 582) costs the same whether its windows are 16 or 256 times larger: grow faster there, the extra speculative tests are free
inline uint64_t fw_pool_growth(size_t n_live, uint64_t launched_ranks, uint64_t forced, uint64_t small_launch)
{
    if (forced) return forced;
    if (launched_ranks < small_launch) return 256;
    return n_live > 2048 ? 4 : 16;
}

// ---- merge and advance ----
// A job's running state between its windows
struct FwJobRun {
    uint64_t N = 0, next = 0, width = 0;
    double best_p = -1.0, best_stat = 0.0;
    uint64_t best_rank = 0;
    int32_t best_df = 0;
    bool done = false;
    bool no_zs = false;  // the returned result has no conditioning set (fz_nz job without a test)
    FwJobOut out{};
};

// One segment record into its job, segments arriving in rank order.  `evaluated` is summed even behind a stop (speculative segments);
// the first stop wins; otherwise the last maximum p (>=: later wins ties, NaN is never taken).
inline void fw_pool_merge(FwJobRun &j, const FwSegOut &so)
{
    j.out.evaluated += (int64_t)so.evaluated;
    if (j.done) return;
    if (so.stop_rank != FW_RANK_NONE) {
        j.out.stat = so.stop_stat;
        j.out.pval = so.stop_pval;
        j.out.df = so.stop_df;
        j.out.suff_power = so.stop_power;
        j.out.status = FW_SUBSETS_STOPPED;
        j.out.num_tests = (int64_t)(so.stop_rank + 1);
        j.best_rank = so.stop_rank;
        j.done = true;
        if (so.stop_df == -2) {
            j.out.df = 0;
            j.out.num_tests = 0;
            j.no_zs = true;
        }
    } else if (so.best_pval >= j.best_p) {
        j.best_p = so.best_pval;
        j.best_stat = so.best_stat;
        j.best_rank = so.best_rank;
        j.best_df = so.best_df;
    }
}

// End of a round for a launched job that did not stop: past its window, the next one `growth` times wider; an exhausted enumeration
// returns the carried maximum (tests.jl:338-345)
inline void fw_pool_advance(FwJobRun &j, uint64_t growth)
{
    j.next += fw_pool_window(j.next, j.width, j.N);
    j.width *= growth;
    if (j.next >= j.N) {
        j.out.stat = j.best_stat;
        j.out.pval = j.best_p < 0.0 ? 0.0 : j.best_p;
        j.out.df = j.best_df;
        j.out.suff_power = 1;
        j.out.status = FW_SUBSETS_ALL_SIG;
        j.out.num_tests = (int64_t)j.N;
        j.done = true;
    }
}
