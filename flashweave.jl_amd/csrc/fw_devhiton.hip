// Device-resident HITON-PC rounds (FW_FZ, FW_MI, FW_MI_NZ).  The host driver of fw_hiton.cpp pays one host round trip per pool round
// (collect -> merge -> advance -> build -> launch, ~140 us at cfg3, a third of the pass); here the per-target state
// machines, the in-rank-order merge of the segment results and the construction of the next launch live in device
// memory and run as three small kernels between two launches of the segment kernel:
//     seg kernel -> dh_step_kernel (merge, commit, advance: one wavefront per target)
//                -> dh_plan_kernel (segment length, per-target segment counts, exclusive scan: one workgroup)
//                -> dh_fill_kernel (one thread per segment record) -> seg kernel -> ...
// (plus dh_compact_kernel once per batch: the three kernels walk a list of the targets that still have work).
// The host only enqueues batches of rounds and looks at a pinned "done" flag between batches.  Semantics are those
// of the host driver (hiton.jl:109-149 interleaving / elimination, check_candidate! :80-107, update_PC_dict! :249-256,
// tests.jl:326-345 merge rules); windows follow the same growth policy.  Speculation here is the look-ahead described
// at dh_step_kernel (elimination phase: next members against the pools they will see if every earlier one is kept;
// interleaving phase: first windows of the next candidates), switched on only while launches are small.
#include <algorithm>
#include <cassert>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "fw_internal.h"
#define MI_MAX_K FW_MAX_K_FAST  // (conditioning sets of 6 and 7 variables: host job pool over the segment kernels of fw_mi.hip)
#include "fw_mi_core.h"
#include "fw_fz_core.h"
#include "fw_unrank.h"

namespace {

struct DhTgt {
    int32_t T, phase, pos, nc;  // nc = candidates of the current phase
    int32_t na, ntpc, npc, wl_n;
    long long co;  // offset of this target's arrays (capacity cap each; accepted list: 2 * co, 2 * cap)
    long long cand_off;  // offset of its interleaving candidates in DhArrays::cand0
    long long wl_off, nb_off;
    int32_t nb_n, cap;
    int32_t jactive, nsp;  // nsp: look-ahead jobs of the elimination phase in the coming launch (see dh_step_kernel)
    int32_t cur, pad0;     // accepted-list buffer in use (0 .. spec_depth)
    unsigned long long jN, jnext, jwidth, jwin, jevaluated;
    unsigned long long c_eval_short;  // executed tests of jobs with at most FW_HK_A accepted variables (FW_TRACE_HOST)
    int na_max, wl_used;              // longest accepted list of any job of this target; whitelisted candidates appended in phase 0
    double jbest_p, jbest_stat;
    unsigned long long c_ref, c_calls, c_eval;  // per-target totals (summed on the host: no same-address atomics)
    double c_alg;
    unsigned int r_first0, r_more0, r_first1, r_more1;  // FW_TRACE_HOST: rounds this target spent on first / later windows of interleaving (0) and elimination (1) jobs
    // look-ahead jobs of the coming launch: spmode 0 = same accepted list / elimination pools, window = the job's own (jwin2 = jwin);
    // spmode 1 = interleaving "assume the current candidate is accepted": list = accepted + [candidate], own first window jwin2 of
    // an enumeration of jN2 subsets (see dh_step_kernel)
    int32_t spmode, wl_unsorted;  // wl_unsorted: the whitelist was appended to on the device (dh_wl_append_kernel): no order, no early exit
    unsigned long long jwin2, jN2;
    long long tm_off;  // fz rounds (r06): offset (floats) of the target's local correlation matrix in DhArrays::tmat, -1: none
};

struct DhGlobal {
    unsigned long long launched_ranks, next_ranks;
    unsigned int n_live_prev, n_live_next;
    unsigned int ns, seglen, done, rounds, rounds_nonempty, max_a;  // max_a: longest accepted list of any job so far
    unsigned long long cond_tests_ref, subsets_calls, evaluated;
    double alg_bytes;
    unsigned int n_act, act_sel;  // unfinished targets: act[act_sel * ntg + 0 .. n_act) (dh_compact_kernel)
    unsigned int pad_b, max_ab;     // max_ab: largest (accepted + whitelisted neighbours still to come) of any target so far: what a
                                    // list can reach without tested acceptances
    unsigned int ns_ring[64];  // segments of the last 64 planned launches (the host reads the record once per batch)
    // words that many workgroups touch: a cache line each
    unsigned int pad_l0[32];
    unsigned int step_ticket;  // (unused: the r05 cooperative round's barrier word)
    unsigned int pad_l1[31];
    unsigned int any_big;      // the coming launch holds a segment with |accepted| > FW_TAB_A (set by the fill): the in-lane variant
                               // of the fz segment kernel leaves at once when it does not
    unsigned int pad_l2[31];
};

// accepted-list buffer b of a target: (spec_depth + 1) buffers of 2 * cap entries each
#define DH_ACC_OFF(x, b, d1) (2ll * (x).co * (long long)(d1) + 2ll * (long long)(b) * (long long)(x).cap)

struct DhArrays {
    const int32_t *cand0;  // interleaving candidates (hiton.jl:211-217 order)
    int32_t *tpc_key, *pc_key, *acc;
    double *tpc_stat, *tpc_p, *pc_stat, *pc_p;
    const int32_t *wl;        // sorted whitelists (feed-forward)
    const unsigned int *wl_cnt;  // device-built whitelists (fwi_devhiton_mi_schedule): entries of variable v's list so far, else null
    const long long *nb_off;  // level-0 neighbour lists (for the empty-pool case, hiton.jl:57-59)
    const int32_t *nb_idx;
    const double *nb_stat, *nb_p;
    const float *tmat;  // fz rounds (r06): the targets' local correlation matrices (DhTgt::tm_off), else null
    fw_rejection *rej;  // rejection log (fw_set_track_rejections): one slot per directed level-0 entry (dh_rej_write), else null
};

struct DhParams {
    double alpha;
    int max_k;
    long long max_tests;
    unsigned long long small_launch, w0_big, w0_small;  // window policy (fw_pool_host.h: fw_pool_first_window / fw_pool_growth)
    unsigned int seg_q, seg_min;                        // segment length granularity / minimum (fz 256 / 256, discrete 4 / 8)
    double disc_bytes_per_col;                          // discrete kinds: n * b / 8 (algorithmic bytes per column), else 0
    int elim_full;                                      // elimination-phase jobs start with the full enumeration as their window
    unsigned long long growth_small, growth, growth_busy;  // window growth: launch below small_launch / default / many jobs
    unsigned int busy_jobs;
    int spec_depth;  // elimination-phase look-ahead: candidates tested ahead of the current one per target (0 = off)
    unsigned long long spec_below;  // ... only while the last launch held fewer ranks than this
    unsigned int mi_seq, mi_win0, mi_chunk_div, mi_chunk_min, mi_chunk_max, mi_help_jobs;  // dh_mi_target_kernel (env knobs)
    unsigned int mi_elim_min;  // elimination-phase jobs with more ranks than this open a board for the whole enumeration at once (0: off)
    unsigned int mi_heavy;     // targets with at least this many candidates never work on other targets' boards (0: off)
    unsigned int mi_seq_heavy; // ... and run this many first tests of a job alone (instead of mi_seq) before they open a board
    unsigned int mi_seq_tail;  // ... and every target this many once the target list is exhausted (idle wavefronts are waiting for work)
    unsigned int mi_chunk_tail, mi_win0_tail;  // ranks per record / first window once the launch is in its tail (idle wavefronts waiting)
    unsigned int mi_ahead;     // R4 kernels: first tests of up to four interleaving candidates in one step (mi_first4); 0: off
    unsigned int mi_team;      // the first mi_team targets of the (heaviest-first) list are run by a whole workgroup each (dh_mi_team)
    unsigned int mi_team_tail;   // team targets publish tail-mode boards (short records, wide first window) from the start
    unsigned int mi_team_steps;  // lock-step rounds of a team job (4 wavefronts x 1 or 4 ranks each) before its enumeration goes to a board
    unsigned int mi_trace;       // take the per-job / per-target clock reads (FW_TRACE_HOST, FW_MI_TICKS builds)
    int spec0_depth;                // interleaving-phase look-ahead (first windows of the next candidates)
    unsigned long long spec0_below;
    unsigned int spec0_jobs;  // ... and fewer live jobs than this
    int spec0_depth_light;          // ... and this many candidates while the last launch held fewer than spec0_light_below ranks
    unsigned long long spec0_light_below;
    int spec1_depth;          // interleaving-phase look-ahead behind a candidate that is about to be accepted (same two conditions)
    int elim_mode;            // fw_learn_opts.elim_mode: 0 fast_elim; 1 fast_elim = false (dh_commit); 2 ... and no update_PC_dict! (dh_advance)
};

// Is v one of the target's whitelisted neighbours?  Called by the whole wavefront with a uniform v: the lanes read 64 entries of
// the (sorted) list at a time and vote -- ONE load latency per 64 entries.  (r02: a binary search, i.e. log2(n) + 1 DEPENDENT global
// loads per call, up to four calls per target and round: a third of dh_step_kernel's 19 us.)
__device__ __forceinline__ bool dh_in_wl(const DhTgt &x, const DhArrays &A, int32_t v)
{
    const int lane = (int)(threadIdx.x & 63u);
    const int32_t *w = A.wl + x.wl_off;
    for (int base = 0; base < x.wl_n; base += 64) {
        const int32_t e = base + lane < x.wl_n ? w[base + lane] : -1;
        if (__ballot(e == v) != 0ull) return true;
        if (!x.wl_unsorted && __shfl(e, 63) > v) return false;  // sorted: nothing further on can match (an invalid last lane reads -1: the loop ends anyway)
    }
    return false;
}

// algorithmic bytes of the first `evaluated` ranks of a job over `a` accepted variables (fwi_alg_bytes, fz form)
__device__ __forceinline__ double dh_alg_bytes(int a, unsigned long long evaluated, int max_k, double disc_bytes_per_col)
{
    double bytes = 0.0, left = (double)evaluated;
    for (int s = max_k; s >= 1 && left > 0.0; --s) {
        double b = 1.0;
        for (int i = 1; i <= s; ++i) b = b * (double)(a - s + i) / (double)i;
        if (a < s) b = 0.0;
        const double cnt = left < b ? left : b;
        bytes += cnt * (disc_bytes_per_col > 0.0 ? (double)(s + 2) * disc_bytes_per_col + 32.0
                                                 : 4.0 * (double)((s + 2) * (s + 1) / 2) + 32.0);
        left -= cnt;
    }
    return bytes;
}

// number of subsets of sizes max_k .. 1 of a accepted variables, capped by max_tests (tests.jl:300-311): 32-bit binomials (no
// 64-bit division, no Float64 estimate) where every term fits -- all of cfg2 / cfg4; the persistent discrete kernel paid for
// three fw_binom_u64 per job
__device__ __forceinline__ unsigned long long dh_enum_size(int a, int max_k, long long max_tests)
{
    unsigned long long N = 0ull;
    if (max_k <= 3 && a <= FW_UNRANK32_A) {
        for (int s = max_k; s >= 1; --s) N += (unsigned long long)fw_binom32(a, s);
    } else {
        for (int s = max_k; s >= 1; --s) {
            N += fw_binom_u64(a, s);
            if (N > (1ull << 62)) N = 1ull << 62;
        }
    }
    if (max_tests > 0 && (unsigned long long)max_tests < N) N = (unsigned long long)max_tests;
    return N;
}

// Rejection log (update_sig_result!, hiton.jl:71-76): the job of (x.T, cand) over acc[0..a) ended with test number nt of its enumeration
// (tests.jl:281-346 order: sizes max_k .. 1, lexicographic positions), and that test is not significant.  ONE lane unranks nt - 1 against
// the list the job ran on and writes the record to the candidate's slot of the target's level-0 list: a fixed address per (target,
// candidate), so neither atomics nor an order between wavefronts are involved.  nt = 0: the job ended without a test (tests.jl:293-296).
// frac is filled in on the host (from n_acc).
__device__ __noinline__ void dh_rej_write(const DhTgt &x, const DhArrays &A, int max_k, int32_t cand, const int32_t *acc, int a,
                                          unsigned long long nt, double stat, double p, int df, int pow)
{
    const int32_t *b = A.nb_idx + x.nb_off;
    int lo = 0, hi = x.nb_n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (b[mid] < cand)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo >= x.nb_n || b[lo] != cand) return;  // (every candidate is a level-0 neighbour: never taken)
    fw_rejection r;
    r.target = x.T;
    r.candidate = cand;
    r.n_zs = 0;
#pragma unroll
    for (int q = 0; q < FW_MAX_K; ++q) r.zs[q] = 0;
    if (nt > 0ull) {
        unsigned long long rem = nt - 1ull;
        int s = max_k;
        while (s > 1) {
            const unsigned long long cnt = fw_binom_u64(a, s);
            if (rem < cnt) break;
            rem -= cnt;
            --s;
        }
        int pos[FW_MAX_K_FAST];
        fw_unrank_comb(rem, a, s, pos);
        r.n_zs = s;
#pragma unroll
        for (int q = 0; q < FW_MAX_K_FAST; ++q)
            if (q < s) r.zs[q] = acc[pos[q]];
    }
    r.df = nt > 0ull ? df : 0;
    r.suff_power = pow;
    r.phase = x.phase;
    r.n_acc = a;
    r.num_tests = (long long)nt;
    r.frac = 0.0;
    r.stat = stat;
    r.pval = p;
    A.rej[x.nb_off + lo] = r;
}

// dh_alg_bytes for the discrete kinds with max_k <= 3 and short lists: the same sum in integers (bytes per test of size s are
// (s + 2) * bytes_per_col + 32, a multiple of 1/8 at most -> exact in Float64 either way)
__device__ __forceinline__ double dh_alg_bytes_disc32(int a, unsigned long long evaluated, int max_k, double disc_bytes_per_col)
{
    double bytes = 0.0;
    unsigned long long left = evaluated;
    for (int s = max_k; s >= 1 && left > 0ull; --s) {
        const unsigned long long b = (unsigned long long)fw_binom32(a, s), cnt = left < b ? left : b;
        bytes += (double)cnt * ((double)(s + 2) * disc_bytes_per_col + 32.0);
        left -= cnt;
    }
    return bytes;
}

// Advance a target until it needs a device test (returns true; the job is (T, cands[pos], acc[0..na))) or finishes.
// Executed by the whole wavefront of the target: every lane holds the same copy of x and takes the same branches
// (stores of one lane are made visible to the others by workgroup-scope fences: one L1 per CU, no cache maintenance);
// the loops over the target's arrays (removing the candidate from the pool, the phase switch, update_PC_dict!) are
// spread over the lanes -- a single lane walking 250 dependent global loads per candidate was 100 us per round.
// keep_elim_stats (elim_mode 2: fast_elim = no_red_tests = false): update_PC_dict! is skipped (hiton.jl:388-390), PC keeps the
// elimination-phase statistics.
__device__ bool dh_advance(DhTgt &x, const DhArrays &A, int lane, int d1, bool keep_elim_stats = false)
{
    for (;;) {
        int32_t *acc = A.acc + DH_ACC_OFF(x, x.cur, d1);
        if (x.phase == 2) return false;
        const int32_t *cands = x.phase == 0 ? A.cand0 + x.cand_off : A.tpc_key + x.co;
        int32_t *dkey = (x.phase == 0 ? A.tpc_key : A.pc_key) + x.co;
        double *dstat = (x.phase == 0 ? A.tpc_stat : A.pc_stat) + x.co;
        double *dp = (x.phase == 0 ? A.tpc_p : A.pc_p) + x.co;
        int32_t &dn = x.phase == 0 ? x.ntpc : x.npc;
        while (x.pos < x.nc) {
            const int32_t cand = cands[x.pos];
            if (x.wl_n > 0 && dh_in_wl(x, A, cand)) {  // hiton.jl:20-30
                if (lane == 0) {
                    acc[x.na] = cand;
                    dkey[dn] = cand;
                    dstat[dn] = NAN;
                    dp[dn] = NAN;
                }
                ++x.na;
                x.wl_used += x.phase == 0 ? 1 : 0;
                ++dn;
                ++x.pos;
                continue;
            }
            if (x.phase == 1) {  // hiton.jl:134-136: the candidate leaves the conditioning pool while it is tested
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                int w = 0;  // stable in-place compaction, 64 entries at a time (writes never pass the read front)
                for (int base = 0; base < x.na; base += 64) {
                    const int q = base + lane;
                    const int32_t v = q < x.na ? acc[q] : cand;
                    const bool keep = q < x.na && v != cand;
                    const unsigned long long m = __ballot(keep);
                    if (keep) acc[w + __popcll(m & ((1ull << lane) - 1ull))] = v;
                    w += __popcll(m);
                }
                x.na = w;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
            }
            if (x.na == 0) {  // tests.jl:285 sentinel + hiton.jl:57-59
                double s = NAN, p = NAN;
                if (x.phase == 0) {
                    const int32_t *b = A.nb_idx + x.nb_off;
                    int lo = 0, hi = x.nb_n;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (b[mid] < cand)
                            lo = mid + 1;
                        else
                            hi = mid;
                    }
                    s = A.nb_stat[x.nb_off + lo];
                    p = A.nb_p[x.nb_off + lo];
                } else {
                    for (int q = 0; q < x.ntpc; ++q)
                        if (A.tpc_key[x.co + q] == cand) {
                            s = A.tpc_stat[x.co + q];
                            p = A.tpc_p[x.co + q];
                            break;
                        }
                }
                if (lane == 0) {
                    acc[x.na] = cand;
                    dkey[dn] = cand;
                    dstat[dn] = s;
                    dp[dn] = p;
                }
                ++x.na;
                ++dn;
                ++x.pos;
                continue;
            }
            return true;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        if (x.phase == 0) {  // hiton.jl:242: elimination over keys(TPC) in insertion order
            x.phase = 1;
            x.nc = x.ntpc;
            for (int q = lane; q < x.ntpc; q += 64) acc[q] = A.tpc_key[x.co + q];
            x.na = x.ntpc;
            x.pos = 0;
        } else {  // hiton.jl:249-256 update_PC_dict! (skipped when fast_elim = no_red_tests = false, hiton.jl:388-390)
            for (int i = keep_elim_stats ? x.npc : lane; i < x.npc; i += 64) {
                const int32_t k = A.pc_key[x.co + i];
                for (int q = 0; q < x.ntpc; ++q)
                    if (A.tpc_key[x.co + q] == k) {
                        const double tp = A.tpc_p[x.co + q], pp = A.pc_p[x.co + i];
                        if (tp > pp || isnan(pp)) {
                            A.pc_stat[x.co + i] = A.tpc_stat[x.co + q];
                            A.pc_p[x.co + i] = tp;
                        }
                        break;
                    }
            }
            x.phase = 2;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    }
}

// ceil(w / seglen) for w < 2^62: double quotient + exact fix-up (a 64-bit integer division costs ~100 instructions)
__device__ __forceinline__ unsigned int dh_ceil_div(unsigned long long w, unsigned long long seglen, double inv)
{
    if (w == 0ull) return 0u;
    unsigned long long q = (unsigned long long)((double)w * inv);
    while (q * seglen < w) ++q;
    while (q > 0ull && (q - 1ull) * seglen >= w) --q;
    return (unsigned int)q;
}


// In-rank-order merge of the nseg segment records of one job by the 64 lanes of a wavefront (tests.jl:326-345): the
// first stop (smallest segment index) ends the job; otherwise the lexicographic maximum of (p, segment index), i.e.
// "later wins ties" (tests.jl:338).  Every lane returns the same values.
#define DH_MAX_SPEC 8  // look-ahead jobs per target (register arrays in dh_step_kernel)
#define DH_SPEC_EXACT 4  // default look-ahead depth of the exact elimination mode (fw_learn_opts.elim_mode != 0)

struct DhMerge {
    bool stop;
    double stat, p;  // of the stopping test (stop) or of the maximum-p test (!stop; p = -2 if no segment had one)
    int pow;
    unsigned long long nt;  // stop: tests up to and including the stopping one
    unsigned long long ev;  // tests executed by the segments
    double g;               // mi_merge, !stop: G^2 and df of the maximum-p test (the seed of later records of the job)
    int df;                 // dh_merge, stop: df of the stopping test (the rejection log)
};

// TR (rejection log): the stopping test's df comes back as well; the default instantiation is the merge as it was
template <bool TR = false>
__device__ __forceinline__ DhMerge dh_merge(const FwSegOut *__restrict__ so, long long base, int nseg, int lane)
{
    unsigned long long ev = 0ull;
    int my_stop = 0x7fffffff;  // smallest segment index of this lane that reports a stop
    double st_stat = 0.0, st_p = 0.0;
    int st_pow = 0, st_df = 0;
    unsigned long long st_rank = 0ull;
    double bp = -2.0, bs = 0.0;  // lane best over its segments (increasing index, `>=`)
    int bi = -1;
    for (int sg = lane; sg < nseg; sg += 64) {
        const FwSegOut o = so[base + sg];
        ev += o.evaluated;
        if (o.stop_rank != FW_RANK_NONE) {
            if (my_stop == 0x7fffffff) {
                my_stop = sg;
                st_stat = o.stop_stat;
                st_p = o.stop_pval;
                st_pow = o.stop_power;
                st_rank = o.stop_rank;
                st_df = o.stop_df;
            }
        } else if (o.best_pval >= bp) {
            bp = o.best_pval;
            bs = o.best_stat;
            bi = sg;
        }
    }
    int first = my_stop;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ev += __shfl_xor(ev, o);
        const int f2 = __shfl_xor(first, o);
        first = f2 < first ? f2 : first;
        const double p2 = __shfl_xor(bp, o), s2 = __shfl_xor(bs, o);
        const int i2 = __shfl_xor(bi, o);
        if (p2 > bp || (p2 == bp && i2 > bi)) {
            bp = p2;
            bs = s2;
            bi = i2;
        }
    }
    DhMerge M;
    M.ev = ev;
    if (first != 0x7fffffff) {  // segments after the first stop were speculative
        const int owner = first & 63;
        M.stop = true;
        M.stat = __shfl(st_stat, owner);
        M.p = __shfl(st_p, owner);
        M.pow = __shfl(st_pow, owner);
        M.nt = __shfl(st_rank, owner) + 1ull;
        // fz_nz: too few rows with T != 0 and candidate != 0 -> (0, 1, 0, false) with ZERO tests (tests.jl:294-296; marker of fz_seg_body)
        if (__shfl(st_df, owner) == -2) M.nt = 0ull;
        if constexpr (TR) M.df = __shfl(st_df, owner);
    } else {
        M.stop = false;
        M.stat = bs;
        M.p = bi >= 0 ? bp : -2.0;
        M.pow = 1;
        M.nt = 0ull;
    }
    M.g = 0.0;
    if constexpr (!TR) M.df = 0;
    else if (!M.stop) M.df = 0;
    return M;
}

// issig (tests.jl:1-3) -> hiton.jl:61-63: the candidate at x.pos joins the accepted list (buffer x.cur) and TPC / PC,
// or is dropped.  Every lane computes the same state; lane 0 writes.  Returns whether the candidate joined the accepted list.
// exact (fast_elim = false, hiton.jl:67-70): a rejected elimination-phase member re-enters the pool all the same, without
// entering PC -- the pool of the next member no longer depends on this verdict.
// TR (rejection log, a compile-time instantiation: the default one is the commit as it was): a rejection -- the stopping test was
// number r_nt of the enumeration, with r_df degrees of freedom -- leaves its record (dh_rej_write).
template <bool TR = false>
__device__ __forceinline__ bool dh_commit(DhTgt &x, const DhArrays &A, int lane, int d1, double r_stat, double r_p, int r_pow,
                                          double alpha, bool exact = false, int max_k_rej = 0, unsigned long long r_nt = 0ull, int r_df = 0)
{
    const int32_t *cands = x.phase == 0 ? A.cand0 + x.cand_off : A.tpc_key + x.co;
    const int32_t cand = cands[x.pos];
    ++x.pos;
    if (!(r_p < alpha && r_pow)) {
        if constexpr (TR) {  // (the list entries were written by this lane or by an earlier kernel: nothing to order)
            if (lane == 0) dh_rej_write(x, A, max_k_rej, cand, A.acc + DH_ACC_OFF(x, x.cur, d1), x.na, r_nt, r_stat, r_p, r_df, r_pow);
        }
        if (!(exact && x.phase == 1)) return false;
        if (lane == 0) A.acc[DH_ACC_OFF(x, x.cur, d1) + x.na] = cand;
        ++x.na;
        return true;
    }
    if (lane == 0) {
        A.acc[DH_ACC_OFF(x, x.cur, d1) + x.na] = cand;
        if (x.phase == 0) {
            A.tpc_key[x.co + x.ntpc] = cand;
            A.tpc_stat[x.co + x.ntpc] = r_stat;
            A.tpc_p[x.co + x.ntpc] = r_p;
        } else {
            A.pc_key[x.co + x.npc] = cand;
            A.pc_stat[x.co + x.npc] = r_stat;
            A.pc_p[x.co + x.npc] = r_p;
        }
    }
    ++x.na;
    if (x.phase == 0)
        ++x.ntpc;
    else
        ++x.npc;
    return true;
}

// ---- discrete kinds: persistent wavefronts, one target at a time, big enumerations shared through a board ---------------
// A discrete (T, candidate) job is a handful of tests (cfg4: 3.3 on average, 786 000 jobs per pass) and a test is a few
// thousand instructions (fw_mi_core.h), so the level-synchronous rounds above (segment kernel -> step -> plan -> fill,
// ~550 dependent rounds per chain at cfg4, a 16-rank speculative window per job) cost more than the tests themselves.
// Here the launch holds as many wavefronts as the GPU keeps resident; each takes the next target of a heaviest-first list
// (one atomic) and runs its whole HITON-PC: dh_advance / dh_commit are the state machine of the rounds (hiton.jl:109-149,
// :53-78, :249-256), test_subsets (tests.jl:281-346) runs sequentially in the reference's own order, so a job that stops
// after a few tests -- nearly all of them -- costs exactly those tests: no window, no speculation, no round trip.
// A job that survives its first mi_seq tests is an enumeration that will probably run to the end (cfg4: one target owns
// a chain of 90 000 tests).  Its owner publishes the following ranks window by window on a BOARD in device memory: chunk
// records any wavefront can claim with one atomic.  Wavefronts look at the boards before every job of their own and when
// they run out of targets, so a big enumeration gets the whole GPU while its owner waits; the owner claims chunks of its
// own board too, which is why nothing ever waits on a wavefront that is not running.  Chunk results are merged in rank
// order exactly like segment records (dh_merge): first stop wins, otherwise the (p, rank) maximum with "later wins
// ties"; a stop found by one chunk cancels the later chunks of the board (stop_min).  num_tests is the reference's count.
// (the thresholds live in DhParams: mi_seq = 48 tests of a job its owner runs alone before it opens a board, mi_win0 = 128 ranks in the
// first board window, later windows grow x8 -- set where the launch parameters are built, with the sweeps that chose them)
#define MI_BOARD_CAP (1u << 18)
#define MI_REC_CAP (1u << 20)

// one LDS table [stratum][cell] per wavefront (fw_mi_core.h); module scope so that the called test routine addresses it as LDS
__shared__ unsigned short dh_mi_tab[4][2 * MI_TAB16];  // (twice the 16-bit table: the 32-bit form of more than 65 535 samples)

__shared__ int32_t dh_mi_acc[4][1024];  // a helper's copy of the accepted list of the board it works on (MI_ACC_LDS)
__shared__ DhTgt dh_mi_x[4];            // the state of the target each wavefront of dh_mi_target_kernel is working on
__shared__ MiBest dh_mi_seed[4];        // the seed a wavefront hands to the test routine (mi_run_ranks)
// Everything the out-of-line routines of the persistent kernel need about the launch -- device arrays, data description, parameters --
// sits in LDS, written once by the kernel, and the test routine leaves its record in its wavefront's LDS slot.  r02 / r03 passed
// MiDev by value and DhArrays / DhParams by reference and returned FwSegOut by value: by-value structs cross a call through
// private memory (100 + 72 bytes PER LANE written and read back per call, 1 M calls per cfg4 pass), and a by-reference kernel
// argument forces the kernel to keep a stack copy that every use in the callee loads from -- the r03 counters showed twice as many
// bytes written as read by this kernel, and the r04 tick profile 9 us per call outside the tests (profiles/r04_cfg4_attribution.json).
struct DhMiCtx {
    DhArrays A;
    MiDev M;
    DhParams P;
};
__shared__ DhMiCtx dh_mi_ctx;
__shared__ FwSegOut dh_mi_out[4];  // the record of the last mi_run_ranks / mi_run_ranks4 call of each wavefront
#ifdef FW_MI_TICKS
__shared__ unsigned long long dh_mi_ticks[4][12];  // per wavefront: calls, tests, ticks in the prologue / the test core / the accounting (Q) / sizes; [6..11]: ticks in dh_advance, job set-up (enumeration size, tail look), commit + counters, publish, wait for own board (idle), merge
#endif

// Everything two wavefronts share travels as write-through messages: the producer stores with sc1 (relaxed agent-scope atomic
// stores: the line leaves its XCD's L2), drains them with `s_waitcnt vmcnt(0)` (inline asm: the compiler drops the builtin
// form after a release fence on ROCm 7.2, MI355X_MICROARCH.md "compiler hazard") and then raises the flag / counter; the
// consumer polls with ONE relaxed sc1 load and reads the payload with sc1 loads.  No acquire / release fences: on this
// multi-XCD part an agent acquire invalidates the reader's L2 -- i.e. the bit planes every test reads -- and the first
// version of this kernel, which fenced per record, ran 15x slower with 2-rank records than with 8-rank ones.
struct MiBoard {
    unsigned long long tc;        // T | cand << 32
    unsigned long long ac;        // a | chunk << 32            (chunk = ranks per record)
    unsigned long long acc_off;   // accepted list of the job: write-through copy in MiShared::bacc
    unsigned long long start, end;  // ranks [start, end) of the window
    unsigned long long nr;        // nch | res_off << 32        (records of the window: res[res_off .. res_off + nch))
    unsigned long long stop_min;  // smallest stopping rank found so far (FW_RANK_NONE: none)
    unsigned int next_chunk, done;  // claimed / finished records
    unsigned int ready, seed_df;
    double seed_p, seed_g;        // the job's maximum-p test so far (seed_p < 0: none): records skip the Q(a, x) of tests it dominates
};

struct alignas(16) MiQueue {
    unsigned int next_target, targets_done, n_boards, hint, res_top, bacc_top, pad[1], next_team;  // pad[0]: watchdog code
    unsigned long long t_body, t_ctl, t_sleep, n_seg;  // dh_mi_target_kernel: 100 MHz ticks summed over wavefronts (FW_TRACE_HOST; see the end of the kernel)
    unsigned long long t_total;  // dh_mi_target_kernel: ticks until the wavefront ran out of targets (the fields above: see its end)
    unsigned long long tick[12];  // FW_MI_TICKS builds: calls of the test routine, tests, ticks before / in the test core / in the accounting, sum of set sizes; [6..11] see dh_mi_ticks
    unsigned long long tm_run, tm_wait, tm_steps, tm_tests;  // dh_mi_team: ticks inside the test routine / at the barrier behind it, lock-step rounds, tests in them (all wavefronts)
};

#define MI_BACC_CAP (1u << 22)  // ints of accepted-list copies per launch
#define MI_ACC_LDS 1024         // accepted-list entries a helper stages in LDS (longer lists are read through sc1 loads)

__device__ __forceinline__ unsigned int mi_ld_u32(const unsigned int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long mi_ld_u64(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mi_st_u64(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mi_st_u32(unsigned int *p, unsigned int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void mi_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// the four hot words of MiQueue (next_target, targets_done, n_boards, hint: its first 16 bytes) in ONE sc1 round trip -- the owner
// of a target looks at them before every fourth job, and four dependent relaxed loads were four round trips of ~2 us
typedef unsigned int mi_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ mi_u32x4 mi_ld_u128(const void *p)
{
    mi_u32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
}
#ifndef MI_NAP_WAIT
#define MI_NAP_WAIT 2  // x 128 cycles between two looks at a board the wavefront waits for
#endif
#ifndef MI_NAP_TAIL
#define MI_NAP_TAIL 32  // (1 / 1: cfg4 159.8 ms, 2 / 32: 156.2 -- and the idle wavefronts stop inflating the instruction counters) x 512 cycles between two looks at the boards once the wavefront has run out of targets
#endif
__device__ __forceinline__ void mi_nap_wait()
{
#pragma unroll
    for (int i = 0; i < MI_NAP_WAIT; ++i) __builtin_amdgcn_s_sleep(2);
}
__device__ __forceinline__ void mi_nap_tail()
{
#pragma unroll
    for (int i = 0; i < MI_NAP_TAIL; ++i) __builtin_amdgcn_s_sleep(8);
}
// Watchdog of the waits of the persistent kernel: a wavefront that waits for another one (records of its board, the end of the launch)
// gives up when the word it watches has not CHANGED for MI_WD_TICKS of the 100 MHz clock (2 s: a record is at most mi_chunk_max = 64
// tests) -- the launch then ends with a code in MiQueue::pad[0] and the host call fails with FW_ERR_DEVICE instead of hanging the GPU.
// The clock (a scalar memory round trip) is read every 256th look only.
#ifndef MI_WD_TICKS
#define MI_WD_TICKS 200000000ull
#endif
struct MiWatch {
    unsigned long long t0;
    unsigned int last, n;
};
__device__ __forceinline__ void mi_watch_begin(MiWatch &w, unsigned int word)
{
    w.t0 = 0ull;
    w.last = word;
    w.n = 0u;
}
__device__ __forceinline__ bool mi_watch_expired(MiWatch &w, unsigned int word)
{
    if (word != w.last) {
        w.last = word;
        w.t0 = 0ull;
        w.n = 0u;
        return false;
    }
    if ((++w.n & 255u) != 0u) return false;
    const unsigned long long now = wall_clock64();
    if (w.t0 == 0ull) {
        w.t0 = now;
        return false;
    }
    return now - w.t0 > MI_WD_TICKS;
}
// lane 0 performs the atomic, every lane gets the value
__device__ __forceinline__ unsigned int mi_wave_add(unsigned int *p, unsigned int v, int lane)
{
    unsigned int r = 0u;
    if (lane == 0) r = atomicAdd(p, v);
    return (unsigned int)__builtin_amdgcn_readfirstlane((int)r);
}

// 64-bit v_readlane
__device__ __forceinline__ unsigned long long mi_rfl_lane64(unsigned long long v, int src)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src), hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// ranks [r0, r1) of the job (T, cand | subsets of acc[0..a)) in enumeration order, one test after the other (whole wavefront).
// Called, not inlined: the kernel reaches it from four places (own jobs, own board, other boards while waiting / between
// jobs / at the end) and four copies of the test made 168 KB of code -- against a 64 KB instruction cache.
// STOP_P: the stopping test's p-value is evaluated (mi_account: need_stop_p) -- the rejection log's second look at a stopping test
template <int L, int NXY, int PRE, bool STOP_P = false>
__device__ __noinline__ void mi_run_ranks(int T, int cand, const int32_t *__restrict__ acc_in, int a, int max_k,
                                          long long max_tests, unsigned long long r0, unsigned long long r1,
                                          const unsigned long long *stop_min_in, int remote_acc, const MiBest *seed_in)
{
    unsigned short *tab = dh_mi_tab[threadIdx.x >> 6];
    const MiDev M = mi_uniform(dh_mi_ctx.M);
    T = __builtin_amdgcn_readfirstlane(T);
    cand = __builtin_amdgcn_readfirstlane(cand);
    a = __builtin_amdgcn_readfirstlane(a);
    max_k = __builtin_amdgcn_readfirstlane(max_k);
    max_tests = (long long)mi_rfl64((unsigned long long)max_tests);
    r0 = mi_rfl64(r0);
    r1 = mi_rfl64(r1);
    const int32_t *acc = (const int32_t *)mi_rfl64((unsigned long long)acc_in);
    const unsigned long long *stop_min = (const unsigned long long *)mi_rfl64((unsigned long long)stop_min_in);
    remote_acc = __builtin_amdgcn_readfirstlane(remote_acc);
    FwSegOut o;
    o.stop_rank = FW_RANK_NONE;
    o.stop_stat = o.stop_pval = 0.0;
    o.best_rank = 0ull;
    o.best_stat = 0.0;
    o.best_pval = -3.0;  // "no test": dh_merge ignores it
    o.stop_df = o.stop_power = o.best_df = o.pad = 0;
    o.evaluated = 0ull;
    int s = max_k;
    // the positions of the running subset: only ever indexed with compile-time constants (unrolled loops), so they live in scalar
    // registers.  r05 indexed them with run-time values (the unranking loop, the step to the next subset): a private array on the
    // stack -- five dword stores per call and two or three DEPENDENT scratch loads per test in the stepping code, and, with the
    // callee-saved registers this out-of-line routine has to park, the 3.65 GB the kernel wrote per cfg4 pass for 86 MB of results
    // (profiles/r06_discrete_kernel_writes.txt)
    int pos[MI_MAX_K];
#pragma unroll
    for (int q = 0; q < MI_MAX_K; ++q) pos[q] = 0;
    if (max_k <= 3 && a <= FW_UNRANK32_A) {
        // every rank of the job fits 28 bits: 32-bit binomials, divisions by constants (fw_unrank.h: ~100 instructions instead of
        // ~1 500 -- the r03 trace of cfg4 showed 9.3 us of prologue per call of this routine, as much as a test)
        uint32_t rem = (uint32_t)r0;
        while (s > 1 && rem >= fw_binom32(a, s)) {
            rem -= fw_binom32(a, s);
            --s;
        }
        int prev = -1;  // fw_unrank_comb32 with static position indices (s <= 3 here)
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (d < s) {
                const int t = s - d, n = a - 1 - prev;
                const uint32_t tot = fw_binom32(n, t);
                const int m = fw_inv_binom32(tot - rem, t, n);
                rem -= tot - fw_binom32(m, t);
                pos[d] = a - m;
                prev = a - m;
            }
    } else {
        unsigned long long rem = r0;
        while (s > 1 && rem >= fw_binom_u64(a, s)) {
            rem -= fw_binom_u64(a, s);
            --s;
        }
        int pm[MI_MAX_K];  // (the general form keeps its array: lists beyond 1 024 entries or max_k 4-5, never at the benchmark sizes)
#pragma unroll
        for (int q = 0; q < MI_MAX_K; ++q) pm[q] = 0;
        fw_unrank_comb(rem, a, s, pm);
#pragma unroll
        for (int q = 0; q < MI_MAX_K; ++q) pos[q] = pm[q];
    }
    // the maximum-p record the job holds so far (seed: what earlier ranks of the job found -- LDS, every lane reads the same words).
    // A test the seed dominates (mi_account: df <= and G^2 >) skips its Q(a, x); without a seed every record pays one Q for its
    // first significant test -- 18-25 us at cfg4, three tests' worth.  A record reports a maximum only if it improved on the seed.
    const MiBest *seed = (const MiBest *)mi_rfl64((unsigned long long)seed_in);
    MiBest mb;
    mb.p = -3.0;
    mb.stat = mb.g = 0.0;
    mb.df = 0;
    if (seed) {
        mb.p = seed->p;
        mb.stat = seed->stat;
        mb.g = seed->g;
        mb.df = seed->df;
    }
#ifdef FW_MI_TICKS
    unsigned long long *tkw = dh_mi_ticks[threadIdx.x >> 6];
    unsigned long long tka = wall_clock64();
    if ((threadIdx.x & 63) == 0) tkw[0] += 1ull;
#endif
    for (unsigned long long r = r0; r < r1; ++r) {
        if (stop_min && mi_ld_u64(stop_min) < r) break;  // an earlier rank already ended the job
        MiZs zs;
#pragma unroll
        for (int q = 0; q < MI_MAX_K; ++q)  // remote_acc: another wavefront's list, read where it was written through (sc1)
            zs.v[q] = (q < s) ? (remote_acc ? __hip_atomic_load(&acc[pos[q]], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : acc[pos[q]]) : 0;
#ifdef FW_MI_TICKS
        const unsigned long long tkb = wall_clock64();
#endif
        MiRes t = mi_test_core<L, NXY, PRE == 1, PRE == 2>(M, T, cand, zs, s, tab);  // PRE: 0 words loaded per batch, 1 register-resident (n <= 6144), 2 32-bit counts (n > 65 535)
        ++o.evaluated;
#ifdef FW_MI_TICKS
        const unsigned long long tkc = wall_clock64();
#endif
        const int ev = mi_account(M, t, max_tests > 0 && r + 1ull >= (unsigned long long)max_tests, mb, STOP_P);  // tests.jl:326-341
#ifdef FW_MI_TICKS
        {
            const unsigned long long tkd = wall_clock64();
            if ((threadIdx.x & 63) == 0) {
                tkw[1] += 1ull;
                tkw[2] += tkb - tka;
                tkw[3] += tkc - tkb;
                tkw[4] += tkd - tkc;
                tkw[5] += (unsigned long long)s;
            }
            tka = tkd;
        }
#endif
        if (ev == 1) {
            o.stop_rank = r;
            o.stop_stat = t.stat;
            o.stop_pval = t.pval;
            o.stop_df = t.df;
            o.stop_power = t.power;
            break;
        }
        if (ev == 2) {
            o.best_pval = mb.p;
            o.best_stat = mb.stat;
            o.best_rank = r;
            o.best_df = mb.df;
            o.stop_stat = mb.g;  // (records without a stop: G^2 of the maximum-p test, the seed of later records)
        }
        // next subset of this size in lexicographic order of the positions, then the next size down (static indices: see above)
        int i = -1, base = 0;  // i: the last position that can still move; base: its new value
#pragma unroll
        for (int q = 0; q < MI_MAX_K; ++q)
            if (q < s && pos[q] != a - s + q) {
                i = q;
                base = pos[q] + 1;
            }
        if (i < 0) {
            --s;
            if (s < 1) break;
#pragma unroll
            for (int q = 0; q < MI_MAX_K; ++q) pos[q] = q;
        } else {
#pragma unroll
            for (int q = 0; q < MI_MAX_K; ++q)
                if (q >= i && q < s) pos[q] = base + (q - i);
        }
    }
    if ((threadIdx.x & 63) == 0) dh_mi_out[threadIdx.x >> 6] = o;  // (every lane holds the same record)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The same enumeration, four subsets per step (mi_test_core4: one DPP row of 16 lanes per test; n <= MI4_N, max_k <= 3, 2 x 2 cells
// per stratum): the four tests of a step are ranks r .. r + 3 of the same size; they are accounted for in rank order exactly as the
// sequential loop would (first stop wins, `>=` maximum before it), so the tests behind a stop inside a step are the only
// speculation (counted in `evaluated`).
template <int L, bool STOP_P = false>
__device__ __noinline__ void mi_run_ranks4(int T, int cand, const int32_t *__restrict__ acc_in, int a, int max_k,
                                           long long max_tests, unsigned long long r0, unsigned long long r1,
                                           const unsigned long long *stop_min_in, int remote_acc, const MiBest *seed_in)
{
    unsigned short *tab = dh_mi_tab[threadIdx.x >> 6];
    const MiDev M = mi_uniform(dh_mi_ctx.M);
    T = __builtin_amdgcn_readfirstlane(T);
    cand = __builtin_amdgcn_readfirstlane(cand);
    a = __builtin_amdgcn_readfirstlane(a);
    max_k = __builtin_amdgcn_readfirstlane(max_k);
    max_tests = (long long)mi_rfl64((unsigned long long)max_tests);
    r0 = mi_rfl64(r0);
    r1 = mi_rfl64(r1);
    const int32_t *acc = (const int32_t *)mi_rfl64((unsigned long long)acc_in);
    const unsigned long long *stop_min = (const unsigned long long *)mi_rfl64((unsigned long long)stop_min_in);
    remote_acc = __builtin_amdgcn_readfirstlane(remote_acc);
    const int row = (threadIdx.x & 63) >> 4;
    FwSegOut o;
    o.stop_rank = FW_RANK_NONE;
    o.stop_stat = o.stop_pval = 0.0;
    o.best_rank = 0ull;
    o.best_stat = 0.0;
    o.best_pval = -3.0;
    o.stop_df = o.stop_power = o.best_df = o.pad = 0;
    o.evaluated = 0ull;
    int s = max_k;
    int p0 = 0, p1 = 0, p2 = 0;  // positions of the running subset (s <= 3), scalar
    {
        int pos[MI_MAX_K];
#pragma unroll
        for (int q = 0; q < MI_MAX_K; ++q) pos[q] = 0;
        if (a <= FW_UNRANK32_A) {  // (max_k <= 3 here: 32-bit binomials, see mi_run_ranks)
            uint32_t rem = (uint32_t)r0;
            while (s > 1 && rem >= fw_binom32(a, s)) {
                rem -= fw_binom32(a, s);
                --s;
            }
            fw_unrank_comb32(rem, a, s, pos);
        } else {
            unsigned long long rem = r0;
            while (s > 1 && rem >= fw_binom_u64(a, s)) {
                rem -= fw_binom_u64(a, s);
                --s;
            }
            fw_unrank_comb(rem, a, s, pos);
        }
        p0 = pos[0];
        p1 = pos[1];
        p2 = pos[2];
    }
    // the maximum-p record the job holds so far (seed: what earlier ranks of the job found -- LDS, every lane reads the same words).
    // A test the seed dominates (mi_account: df <= and G^2 >) skips its Q(a, x); without a seed every record pays one Q for its
    // first significant test -- 18-25 us at cfg4, three tests' worth.  A record reports a maximum only if it improved on the seed.
    const MiBest *seed = (const MiBest *)mi_rfl64((unsigned long long)seed_in);
    MiBest mb;
    mb.p = -3.0;
    mb.stat = mb.g = 0.0;
    mb.df = 0;
    if (seed) {
        mb.p = seed->p;
        mb.stat = seed->stat;
        mb.g = seed->g;
        mb.df = seed->df;
    }
    unsigned long long r = r0;
    while (r < r1 && s >= 1) {
        if (stop_min && mi_ld_u64(stop_min) < r) break;  // an earlier rank already ended the job
        // up to four subsets of size s: row t takes the t-th; rows beyond the step's count repeat the first (ignored)
        int zrow[3] = {0, 0, 0};
        int nb = 0;
        const int s_step = s;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const bool have = r + (unsigned long long)t < r1 && s == s_step;  // uniform
            if (have) {
                ++nb;
                const int q0 = p0, q1 = s_step >= 2 ? p1 : p0, q2 = s_step >= 3 ? p2 : p0;
                const int v0 = remote_acc ? __hip_atomic_load(&acc[q0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : acc[q0];
                const int v1 = remote_acc ? __hip_atomic_load(&acc[q1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : acc[q1];
                const int v2 = remote_acc ? __hip_atomic_load(&acc[q2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : acc[q2];
                if (row == t || t == 0) {  // t == 0 first: the default of every row
                    zrow[0] = v0;
                    zrow[1] = v1;
                    zrow[2] = v2;
                }
                // next subset in lexicographic order of the positions, then the next size down (scalar)
                if (s_step == 1) {
                    if (p0 < a - 1) ++p0; else s = 0;
                } else if (s_step == 2) {
                    if (p1 < a - 1) {
                        ++p1;
                    } else if (p0 < a - 2) {
                        ++p0;
                        p1 = p0 + 1;
                    } else {
                        s = 1;
                        p0 = 0;
                    }
                } else {
                    if (p2 < a - 1) {
                        ++p2;
                    } else if (p1 < a - 2) {
                        ++p1;
                        p2 = p1 + 1;
                    } else if (p0 < a - 3) {
                        ++p0;
                        p1 = p0 + 1;
                        p2 = p0 + 2;
                    } else {
                        s = 2;
                        p0 = 0;
                        p1 = 1;
                    }
                }
            }
        }
        MiRes mine = mi_test_core4<L>(M, T, cand, zrow, s_step, tab, cand);
        o.evaluated += (unsigned long long)nb;
        bool stopped = false;
        for (int t = 0; t < nb; ++t) {  // rank order (uniform: every lane reads row t's result)
            MiRes tt;
            const int src = 16 * t;
            tt.stat = __longlong_as_double((long long)mi_rfl_lane64((unsigned long long)__double_as_longlong(mine.stat), src));
            tt.g = __longlong_as_double((long long)mi_rfl_lane64((unsigned long long)__double_as_longlong(mine.g), src));
            tt.pval = __longlong_as_double((long long)mi_rfl_lane64((unsigned long long)__double_as_longlong(mine.pval), src));
            tt.df = __builtin_amdgcn_readlane(mine.df, src);
            tt.power = __builtin_amdgcn_readlane(mine.power, src);
            tt.n_obs = (long long)mi_rfl_lane64((unsigned long long)mine.n_obs, src);
            const unsigned long long rr = r + (unsigned long long)t;
            const int ev = mi_account(M, tt, max_tests > 0 && rr + 1ull >= (unsigned long long)max_tests, mb, STOP_P);  // tests.jl:326-341
            if (ev == 1) {
                o.stop_rank = rr;
                o.stop_stat = tt.stat;
                o.stop_pval = tt.pval;
                o.stop_df = tt.df;
                o.stop_power = tt.power;
                stopped = true;
                break;
            }
            if (ev == 2) {
                o.best_pval = mb.p;
                o.best_stat = mb.stat;
                o.best_rank = rr;
                o.best_df = mb.df;
                o.stop_stat = mb.g;  // (records without a stop: G^2 of the maximum-p test, the seed of later records)
            }
        }
        if (stopped) break;
        r += (unsigned long long)nb;
    }
    if ((threadIdx.x & 63) == 0) dh_mi_out[threadIdx.x >> 6] = o;  // (every lane holds the same record)
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- first tests of four candidates at once (R4 kernels) ------------------------------------------------------------------------
// Most interleaving jobs end with their FIRST test (cfg2: 2.6 tests per job, a target with 190 candidates is a chain of ~200 jobs of
// ~20 us).  While a candidate is rejected the accepted list does not change, so the first test of the next candidates -- (T, c | the
// first subset of the same list) -- can be evaluated before the current one is decided: one mi_test_core4 step takes candidates
// pos .. pos + 3 on its four rows (same X, same Z, the row's own Y).  The results are kept per wavefront and consumed in
// candidate order as long as (target, accepted length) still match; the first accepted candidate invalidates the rest.  A
// candidate whose first test is significant continues with rank 1 of its own job, seeded with that test.
struct MiAhead {
    int T, pos0, na, n;  // results for candidates pos0 .. pos0 + n - 1 of target T's interleaving list, accepted length na
    int stop[4], df[4], power[4];
    double stat[4], pval[4], g[4];  // stop: the test ended the job (stat / pval / df / power of it); else its p is materialised
};
__shared__ MiAhead dh_mi_ahead[4];

// candidates cands[0 .. nb) that can share ONE mi_test_core4 step with the first of them: the uniform decisions of the test core read
// levels / maxv > 1 of Y, so only candidates that agree with cands[0] on both ride along (uniform: every lane computes the same count)
__device__ __forceinline__ int mi_first_run(const MiDev &M, const int32_t *__restrict__ cands, int nb)
{
    const int c0 = cands[0];
    int n = 1;
    for (int t = 1; t < nb; ++t) {
        const int ct = cands[t];
        if (M.levels[ct] != M.levels[c0] || (M.maxv[ct] > 1) != (M.maxv[c0] > 1)) break;
        ++n;
    }
    return n;
}

template <int L>
__device__ __noinline__ void mi_first4(int T, int pos0, const int32_t *__restrict__ cands_in, int nb, const int32_t *__restrict__ acc_in,
                                       int a, int max_k, long long max_tests)
{
    unsigned short *tab = dh_mi_tab[threadIdx.x >> 6];
    MiAhead &H = dh_mi_ahead[threadIdx.x >> 6];
    const MiDev M = mi_uniform(dh_mi_ctx.M);
    T = __builtin_amdgcn_readfirstlane(T);
    pos0 = __builtin_amdgcn_readfirstlane(pos0);
    nb = __builtin_amdgcn_readfirstlane(nb);
    a = __builtin_amdgcn_readfirstlane(a);
    max_k = __builtin_amdgcn_readfirstlane(max_k);
    max_tests = (long long)mi_rfl64((unsigned long long)max_tests);
    const int32_t *cands = (const int32_t *)mi_rfl64((unsigned long long)cands_in);
    const int32_t *acc = (const int32_t *)mi_rfl64((unsigned long long)acc_in);
    const int lane = threadIdx.x & 63, row = lane >> 4;
    const int s = max_k < a ? max_k : a;  // rank 0: the first subset of the largest size the list allows (tests.jl:300-311)
    int zrow[3];
    zrow[0] = acc[0];
    zrow[1] = acc[s >= 2 ? 1 : 0];
    zrow[2] = acc[s >= 3 ? 2 : 0];
    const int c0 = cands[0];
    const int n = mi_first_run(M, cands, nb);
    const int my_c = cands[row < n ? row : 0];
    MiRes mine = mi_test_core4<L>(M, T, c0, zrow, s, tab, my_c);
    for (int t = 0; t < n; ++t) {
        MiRes tt;
        const int src = 16 * t;
        tt.stat = __longlong_as_double((long long)mi_rfl_lane64((unsigned long long)__double_as_longlong(mine.stat), src));
        tt.g = __longlong_as_double((long long)mi_rfl_lane64((unsigned long long)__double_as_longlong(mine.g), src));
        tt.pval = __longlong_as_double((long long)mi_rfl_lane64((unsigned long long)__double_as_longlong(mine.pval), src));
        tt.df = __builtin_amdgcn_readlane(mine.df, src);
        tt.power = __builtin_amdgcn_readlane(mine.power, src);
        tt.n_obs = (long long)mi_rfl_lane64((unsigned long long)mine.n_obs, src);
        MiBest mb;
        mb.p = -3.0;
        mb.stat = mb.g = 0.0;
        mb.df = 0;
        const int ev = mi_account(M, tt, max_tests == 1, mb, false);  // tests.jl:326-341 for rank 0
        if (lane == 0) {
            H.stop[t] = ev == 1;
            H.stat[t] = tt.stat;
            H.pval[t] = ev == 1 ? tt.pval : mb.p;
            H.g[t] = tt.g;
            H.df[t] = tt.df;
            H.power[t] = tt.power;
        }
    }
    if (lane == 0) {
        H.T = T;
        H.pos0 = pos0;
        H.na = a;
        H.n = n;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// R4: the four-subsets-per-step form (host: n <= MI4_N, max_k <= 3, 2 x 2 cells); one of the two routines per instantiation
template <int L, int NXY, int PRE, bool R4, bool STOP_P = false>
__device__ __forceinline__ FwSegOut mi_run_ranks_sel(int T, int cand, const int32_t *__restrict__ acc, int a, int max_k,
                                                     long long max_tests, unsigned long long r0, unsigned long long r1,
                                                     const unsigned long long *stop_min, int remote_acc, const MiBest *seed)
{
    if constexpr (R4)
        mi_run_ranks4<L, STOP_P>(T, cand, acc, a, max_k, max_tests, r0, r1, stop_min, remote_acc, seed);
    else
        mi_run_ranks<L, NXY, PRE, STOP_P>(T, cand, acc, a, max_k, max_tests, r0, r1, stop_min, remote_acc, seed);
    return dh_mi_out[threadIdx.x >> 6];  // (inlined: the record comes back through LDS, not through a by-value return)
}

// one record = 9 64-bit words (FwSegOut), written through / read back word by word
__device__ __forceinline__ void mi_record_store(FwSegOut *dst, const FwSegOut &o)
{
    unsigned long long w[9];
    __builtin_memcpy(w, &o, sizeof(w));
    unsigned long long *d = (unsigned long long *)dst;
#pragma unroll
    for (int q = 0; q < 9; ++q) mi_st_u64(d + q, w[q]);
}
__device__ __forceinline__ FwSegOut mi_record_load(const FwSegOut *src)
{
    unsigned long long w[9];
    const unsigned long long *d = (const unsigned long long *)src;
#pragma unroll
    for (int q = 0; q < 9; ++q) w[q] = mi_ld_u64(d + q);
    FwSegOut o;
    __builtin_memcpy(&o, w, sizeof(w));
    return o;
}
static_assert(sizeof(FwSegOut) == 72, "FwSegOut is nine 64-bit words");

// dh_merge over records another wavefront wrote through (sc1 loads)
__device__ __forceinline__ DhMerge mi_merge(const FwSegOut *__restrict__ so, long long base, int nseg, int lane)
{
    unsigned long long ev = 0ull;
    int my_stop = 0x7fffffff;
    double st_stat = 0.0, st_p = 0.0;
    int st_pow = 0;
    unsigned long long st_rank = 0ull;
    double bp = -2.0, bs = 0.0, bg = 0.0;
    int bi = -1, bdf = 0;
    for (int sg = lane; sg < nseg; sg += 64) {
        const FwSegOut o = mi_record_load(so + base + sg);
        ev += o.evaluated;
        if (o.stop_rank != FW_RANK_NONE) {
            if (my_stop == 0x7fffffff) {
                my_stop = sg;
                st_stat = o.stop_stat;
                st_p = o.stop_pval;
                st_pow = o.stop_power;
                st_rank = o.stop_rank;
            }
        } else if (o.best_pval >= bp) {
            bp = o.best_pval;
            bs = o.best_stat;
            bg = o.stop_stat;  // (records without a stop carry the G^2 of their maximum here)
            bdf = o.best_df;
            bi = sg;
        }
    }
    int first = my_stop;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ev += __shfl_xor(ev, o);
        const int f2 = __shfl_xor(first, o);
        first = f2 < first ? f2 : first;
        const double p2 = __shfl_xor(bp, o), s2 = __shfl_xor(bs, o), g2 = __shfl_xor(bg, o);
        const int i2 = __shfl_xor(bi, o), d2 = __shfl_xor(bdf, o);
        if (p2 > bp || (p2 == bp && i2 > bi)) {
            bp = p2;
            bs = s2;
            bg = g2;
            bdf = d2;
            bi = i2;
        }
    }
    DhMerge M;
    M.ev = ev;
    if (first != 0x7fffffff) {
        const int owner = first & 63;
        M.stop = true;
        M.stat = __shfl(st_stat, owner);
        M.p = __shfl(st_p, owner);
        M.pow = __shfl(st_pow, owner);
        M.nt = __shfl(st_rank, owner) + 1ull;
    } else {
        M.stop = false;
        M.stat = bs;
        M.p = bi >= 0 ? bp : -2.0;
        M.pow = 1;
        M.nt = 0ull;
    }
    M.g = bg;
    M.df = bdf;
    return M;
}

// claim and evaluate one record of board b (if any is left); true if a record was processed.  acc_own: the caller published the board (its accepted list is at hand); otherwise the list is
// staged from the board's write-through copy.
template <int L, int NXY, int PRE, bool R4>
__device__ __forceinline__ bool mi_board_work(MiBoard *__restrict__ b, FwSegOut *__restrict__ res, const int32_t *__restrict__ bacc,
                                              const int32_t *acc_own, int lane)
{
    const DhParams &P = dh_mi_ctx.P;
    const unsigned long long nr = mi_ld_u64(&b->nr);
    const unsigned int nch = (unsigned int)nr, res_off = (unsigned int)(nr >> 32);
    if (mi_ld_u32(&b->next_chunk) >= nch) return false;
    const unsigned int c = mi_wave_add(&b->next_chunk, 1u, lane);
    if (c >= nch) return false;
    const unsigned long long tc = mi_ld_u64(&b->tc), ac = mi_ld_u64(&b->ac);
    const int a = (int)(unsigned int)ac, chunk = (int)(unsigned int)(ac >> 32);
    const unsigned long long start = mi_ld_u64(&b->start), end = mi_ld_u64(&b->end);
    const unsigned long long r0 = start + (unsigned long long)c * (unsigned long long)chunk;
    unsigned long long r1 = r0 + (unsigned long long)chunk;
    if (r1 > end) r1 = end;
    FwSegOut o;
    if (mi_ld_u64(&b->stop_min) < r0) {  // cancelled: an earlier rank stopped the job
        o.stop_rank = FW_RANK_NONE;
        o.stop_stat = o.stop_pval = 0.0;
        o.best_rank = 0ull;
        o.best_stat = 0.0;
        o.best_pval = -3.0;
        o.stop_df = o.stop_power = o.best_df = o.pad = 0;
        o.evaluated = 0ull;
    } else {
        const int32_t *acc = acc_own;
        int remote = 0;
        if (!acc_own) {
            const int32_t *src = bacc + mi_ld_u64(&b->acc_off);
            if (a <= MI_ACC_LDS) {  // one coalesced sc1 sweep into this wavefront's LDS slot
                int32_t *slot = dh_mi_acc[threadIdx.x >> 6];
                for (int i = lane; i < a; i += 64) slot[i] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
                acc = slot;
            } else {
                acc = src;
                remote = 1;
            }
        }
        const MiBest *seed = nullptr;
        const double sp = __longlong_as_double((long long)mi_ld_u64((const unsigned long long *)&b->seed_p));
        if (sp >= 0.0) {
            MiBest &sd = dh_mi_seed[threadIdx.x >> 6];
            sd.p = sp;
            sd.stat = 0.0;  // (never reported: a record reports a maximum only if one of its own tests reaches the seed's p)
            sd.g = __longlong_as_double((long long)mi_ld_u64((const unsigned long long *)&b->seed_g));
            sd.df = (int)mi_ld_u32(&b->seed_df);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            seed = &sd;
        }
        o = mi_run_ranks_sel<L, NXY, PRE, R4>((int)(unsigned int)tc, (int)(unsigned int)(tc >> 32), acc, a, P.max_k, P.max_tests, r0, r1,
                                      &b->stop_min, remote, seed);
        if (o.stop_rank != FW_RANK_NONE && lane == 0) atomicMin(&b->stop_min, o.stop_rank);
    }
    if (lane == 0) {
        mi_record_store(res + res_off + c, o);
        mi_drain();  // the record before the count
        atomicAdd(&b->done, 1u);
    }
    return true;
}

// look for an open board (from the first one that still has unclaimed records) and work on one record of it; true if
// something was done.  (A global FIFO of records with a compare-and-swap head was tried instead of the scan: 10x slower --
// a thousand wavefronts polling and swapping the same two words.)
template <int L, int NXY, int PRE, bool R4>
__device__ __noinline__ bool mi_help_scan(MiQueue *__restrict__ Q, MiBoard *__restrict__ boards, FwSegOut *__restrict__ res,
                                          const int32_t *__restrict__ bacc, int lane, unsigned int nb, unsigned int i)
{
    for (; i < nb; ++i) {
        MiBoard *b = boards + i;
        if (mi_ld_u32(&b->ready) == 0u) return false;  // reserved, not yet filled
        if (mi_ld_u32(&b->next_chunk) < (unsigned int)mi_ld_u64(&b->nr)) {
            if (mi_board_work<L, NXY, PRE, R4>(b, res, bacc, nullptr, lane)) return true;
        } else if (i == mi_ld_u32(&Q->hint) && lane == 0) {
            atomicMax(&Q->hint, i + 1u);  // every record of this board is taken: later scans start behind it
        }
    }
    return false;
}
// The look that finds nothing -- no board behind the hint: what a wavefront that has run out of targets sees thousands of times while
// the last heavy targets finish -- stays in the caller.  r05 made the call first: the out-of-line scan keeps ~38 values in callee-saved
// registers across its own call of the test routine and parks them on the stack in its prologue, so every empty poll wrote and read
// back 38 x 256 bytes of scratch (profiles/r06_discrete_kernel_writes.txt).
template <int L, int NXY, int PRE, bool R4>
__device__ __forceinline__ bool mi_help(MiQueue *__restrict__ Q, MiBoard *__restrict__ boards, FwSegOut *__restrict__ res,
                                        const int32_t *__restrict__ bacc, int lane)
{
    unsigned int nb = mi_ld_u32(&Q->n_boards);
    if (nb > MI_BOARD_CAP) nb = MI_BOARD_CAP;
    const unsigned int i = mi_ld_u32(&Q->hint);
    if (i >= nb) return false;
    if (mi_ld_u32(&boards[i].ready) == 0u) return false;  // reserved, not yet filled (the scan would return at once)
    return mi_help_scan<L, NXY, PRE, R4>(Q, boards, res, bacc, lane, nb, i);
}

// ---- heavy targets: one WORKGROUP per target -------------------------------------------------------------------------------------
// cfg4's last feed-forward round (r03 trace, `FW_TRACE_HOST`): the six targets that finish last (126-196 candidates, ~200 jobs each)
// are taken at t = 0 and end at 39-49 ms of a 48 ms launch, 21 ms of it in the owner's sequential prefixes (16 tests x 7 us, one after
// the other) and 26 ms in board phases of ~40 tests in which helpers arrive late (every other wavefront is inside a prefix of its own).
// The chain of such a target is the launch.  So the first mi_team targets of the heaviest-first list get the four wavefronts of a
// workgroup: the leader (wavefront 0) runs the state machine; every job starts with lock-step rounds in which wavefront w evaluates
// rank(s) base + w (the records meet in LDS and are merged in rank order exactly like board records: first stop wins, else the
// `>=` maximum), and what is left of a long enumeration goes to a board as before -- with three helpers that are there at once.
struct MiTeamJob {
    int go, cand, a, tail;
    int hw;                   // R4: the MiAhead slot that already holds this job's first test (-1: none) -- decided by the leader alone
    long long acc_off;
    unsigned long long N;
    unsigned int board;       // board of the current window (MI_BOARD_CAP: none, the leader ran the window alone)
    DhMerge mg;               // merged outcome of the current window
};
__shared__ MiTeamJob dh_mi_tj;
__shared__ FwSegOut dh_mi_trec[2][4];

// allocate + publish a board for ranks [next, next + W) of the job; returns false if the launch is out of board / record space
__device__ __forceinline__ bool mi_publish(MiQueue *__restrict__ Q, MiBoard *__restrict__ boards, int32_t *__restrict__ bacc, unsigned int &bacc_off,
                                           const int32_t *__restrict__ acc, int a, int T, int cand, unsigned long long next, unsigned long long W,
                                           unsigned long long chunk, unsigned int nch, int lane, unsigned int &bi, unsigned int &ro,
                                           double seed_p, double seed_g, int seed_df)
{
    bi = MI_BOARD_CAP;
    ro = MI_REC_CAP;
    if (bacc_off == MI_BACC_CAP && mi_ld_u32(&Q->bacc_top) + (unsigned int)a <= MI_BACC_CAP) {
        bacc_off = mi_wave_add(&Q->bacc_top, (unsigned int)a, lane);
        if (bacc_off + (unsigned int)a > MI_BACC_CAP) {
            bacc_off = MI_BACC_CAP;
        } else {
            for (int i = lane; i < a; i += 64) __hip_atomic_store(bacc + bacc_off + i, acc[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (bacc_off != MI_BACC_CAP && mi_ld_u32(&Q->n_boards) < MI_BOARD_CAP && mi_ld_u32(&Q->res_top) + nch <= MI_REC_CAP) {
        ro = mi_wave_add(&Q->res_top, nch, lane);
        if (ro + nch <= MI_REC_CAP) bi = mi_wave_add(&Q->n_boards, 1u, lane);
    }
    if (bi >= MI_BOARD_CAP) return false;
    MiBoard *b = boards + bi;
    mi_drain();  // the copy of the accepted list (every lane's stores) ...
    if (lane == 0) {
        mi_st_u64(&b->tc, (unsigned long long)(unsigned int)T | ((unsigned long long)(unsigned int)cand << 32));
        mi_st_u64(&b->ac, (unsigned long long)(unsigned int)a | ((unsigned long long)chunk << 32));
        mi_st_u64(&b->acc_off, (unsigned long long)bacc_off);
        mi_st_u64(&b->start, next);
        mi_st_u64(&b->end, next + W);
        mi_st_u64(&b->nr, (unsigned long long)nch | ((unsigned long long)ro << 32));
        mi_st_u64(&b->stop_min, FW_RANK_NONE);  // next_chunk / done are zero from the launch's memset
        mi_st_u64((unsigned long long *)&b->seed_p, (unsigned long long)__double_as_longlong(seed_p > 1e-290 ? seed_p : -1.0));  // (p = 0 seeds nothing: ties)
        mi_st_u64((unsigned long long *)&b->seed_g, (unsigned long long)__double_as_longlong(seed_g));
        mi_st_u32(&b->seed_df, (unsigned int)seed_df);
        mi_drain();  // ... and the board before the flag
        mi_st_u32(&b->ready, 1u);
    }
    return true;
}

// the whole HITON-PC of target t on the four wavefronts of this workgroup (every wavefront calls it; uniform control flow
// between the barriers: every decision is taken from LDS values all four read)
// the persistent kernel's own clock reads (per job: phase times for FW_TRACE_HOST): a wall_clock64() is a scalar memory round trip,
// four of them per job were ~5 % of a light job -- taken only when the host asks for the trace (DhParams::mi_trace)
#define MI_CLK() (P.mi_trace ? wall_clock64() : 0ull)
// Rejection log of the persistent kernel (TR instantiations only): the verdict of a job carries the stopping test's statistic and
// power through the look-ahead slots, the lock-step records and the boards, but neither its degrees of freedom nor its p-value (HITON-PC
// drops a rejected candidate without looking at p, so mi_account does not evaluate Q(a, x) for it) -- the stopping test (rank nt - 1 of
// the enumeration over acc[0..a), the list the job ran on) is evaluated once more by this wavefront, with its p-value, and lane 0
// writes the record (dh_rej_write).  One extra test per rejected candidate, in the tracking instantiations only.
template <int L, int NXY, int PRE, bool R4>
__device__ __forceinline__ void mi_rej_record(MiQueue *__restrict__ Q, const DhTgt &x, int T, int cand, const int32_t *acc, int a, unsigned long long nt,
                                              double r_stat, double r_p, int r_pow, int lane)
{
    const DhArrays &A = dh_mi_ctx.A;
    const DhParams &P = dh_mi_ctx.P;
    const FwSegOut q = mi_run_ranks_sel<L, NXY, PRE, R4, true>(T, cand, acc, a, P.max_k, P.max_tests, nt - 1ull, nt, nullptr, 0, nullptr);
    // the same arithmetic on the same words: the test stops again.  If it ever did not, the record would carry another test's p and df:
    // the launch is failed through the queue's error word (like the watchdogs), nothing is written
    if (q.stop_rank == FW_RANK_NONE) {
        if (lane == 0) atomicExch(&Q->pad[0], 4u);
        return;
    }
    if (lane == 0) dh_rej_write(x, A, P.max_k, cand, acc, a, nt, r_stat, q.stop_pval, q.stop_df, r_pow);
}
template <int L, int NXY, int PRE, bool R4, bool EX, bool TR>
__device__ __noinline__ void dh_mi_team(DhTgt *__restrict__ tg, int ntg, int t, MiQueue *__restrict__ Q,
                                        MiBoard *__restrict__ boards, FwSegOut *__restrict__ res, int32_t *__restrict__ bacc)
{
    const DhArrays &A = dh_mi_ctx.A;
    const DhParams &P = dh_mi_ctx.P;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    DhTgt &x = dh_mi_x[0];
    MiTeamJob &J = dh_mi_tj;
    if (wave == 0 && lane == 0) {
        x = tg[t];
        if (A.wl_cnt) x.wl_n = (int32_t)A.wl_cnt[x.T];  // device-built whitelist: what the earlier launches of the schedule appended
        x.r_first0 = (unsigned int)MI_CLK();
    }
    __syncthreads();
    const unsigned long long per = R4 ? 4ull : 1ull;  // ranks per wavefront and lock-step round
    for (;;) {
        if (wave == 0) {
            const bool more = dh_advance(x, A, lane, 1, (EX || TR) && P.elim_mode == 2);
            if (lane == 0) {
                J.go = more ? 1 : 0;
                if (more) {
                    const int32_t *cands = x.phase == 0 ? A.cand0 + x.cand_off : A.tpc_key + x.co;
                    J.cand = cands[x.pos];
                    J.acc_off = DH_ACC_OFF(x, x.cur, 1);
                    J.a = x.na;
                    J.N = dh_enum_size(x.na, P.max_k, P.max_tests);
                    J.tail = (P.mi_team_tail || (mi_ld_u32(&Q->next_target) + P.mi_team >= (unsigned int)ntg &&
                                                 ((unsigned int)ntg - mi_ld_u32(&Q->targets_done)) * 8u <= gridDim.x * 4u)) ? 1 : 0;
                    // Which look-ahead slot (if any) holds this job's first test is decided HERE, by the leader, between the barrier that
                    // ends the previous job and the one that starts this one: no wavefront writes a slot in that interval.  (r05 let every
                    // wavefront scan the slots inside the job, while wavefront 0 could already be rewriting its own in mi_first4: a late
                    // wavefront then saw the NEW slot 0, skipped the compute branch and its barrier, and ran one barrier behind the others
                    // from there on -- one of the two races behind the pass-to-pass differences of profiles/r05_discrete_pass_to_pass.txt.)
                    int hw = -1;
                    if (R4 && P.mi_ahead && x.phase == 0 && x.na >= 1 && J.N >= 1ull) {
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            const MiAhead &Hq = dh_mi_ahead[w];
                            if (Hq.n > 0 && Hq.T == x.T && Hq.na == x.na && x.pos >= Hq.pos0 && x.pos < Hq.pos0 + Hq.n) hw = w;
                        }
                    }
                    J.hw = hw;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (wave == 0 && J.go && J.a <= MI_ACC_LDS) {  // the job's accepted list: one LDS copy for the four wavefronts (the leader wrote the
            const int32_t *src = A.acc + J.acc_off;    // global one itself: the others must not meet it in a cache of their own)
            for (int i = lane; i < J.a; i += 64) dh_mi_acc[0][i] = src[i];
        }
        __syncthreads();
        if (!J.go) break;
        const int cand = J.cand, a = J.a, T = x.T;
        const int32_t *acc = a <= MI_ACC_LDS ? (const int32_t *)dh_mi_acc[0] : A.acc + J.acc_off;
        const unsigned long long N = J.N;
        const unsigned long long tk1 = MI_CLK();
        // lock-step rounds: wavefront w takes ranks next + w * per ...
        unsigned long long next = 0ull, ev = 0ull, nt = 0ull;
        bool stopped = false;
        double r_stat = 0.0, r_p = 0.0, best_p = -1.0, best_stat = 0.0, best_g = 0.0;
        int r_pow = 1, best_df = 0;
        unsigned int n_rounds = 0u;
        if constexpr (R4) {
            // First tests of up to SIXTEEN candidates in one round (r05; the one-wavefront form of this is mi_first4 in the kernel below).
            // A heavy target of cfg2 is a chain of ~400 jobs of which ~390 end with their first test: while candidates are rejected the
            // accepted list does not change, so the first test of the next candidates -- (T, c | the first subset of the same list) --
            // does not depend on the earlier verdicts.  The four wavefronts take consecutive slices of the candidate list (a slice: up to
            // four candidates that can share a mi_test_core4 step, cut in front of a whitelisted one: it joins without a test and changes
            // the list), the results stay in the wavefronts' MiAhead slots and are consumed in candidate order while (target, accepted
            // length) still match; an accepted candidate invalidates the rest.  r04: every job of a team target started with a
            // lock-step round of 16 ranks of ITS OWN enumeration, 15 of them behind the stop (cfg2: 946 000 executed tests for 287 000).
            if (P.mi_ahead && x.phase == 0 && a >= 1 && N >= 1ull) {
                const int32_t *cands = A.cand0 + x.cand_off;
                int hw = J.hw;  // (the leader's decision: see where J is written)
                unsigned long long computed = 0ull;
                if (hw < 0 && x.nc - x.pos >= 2) {  // (uniform: x and J do not change between the job's first barrier and the one in front of its commit)
                    const MiDev Mu = mi_uniform(dh_mi_ctx.M);
                    int start = x.pos, my_start = x.pos, my_n = 0;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const int nb = x.nc - start < 4 ? x.nc - start : 4;
                        if (nb <= 0) break;
                        int n = mi_first_run(Mu, cands + start, nb);  // (a cut by the levels only ends the slice: the next wavefront goes on)
                        bool wl_cut = false;
                        if (x.wl_n > 0)  // a whitelisted candidate ends the chain of first tests (the candidate at x.pos itself is not one: dh_advance)
                            for (int q = (start == x.pos ? 1 : 0); q < n; ++q)
                                if (dh_in_wl(x, A, cands[start + q])) {
                                    n = q;
                                    wl_cut = true;
                                    break;
                                }
                        if (w == wave) {
                            my_start = start;
                            my_n = n;
                        }
                        start += n;
                        if (wl_cut) break;
                    }
                    computed = (unsigned long long)(start - x.pos);
                    if (my_n > 0)
                        mi_first4<L>(T, my_start, cands + my_start, my_n, acc, a, P.max_k, P.max_tests);
                    else if (lane == 0)
                        dh_mi_ahead[wave].n = 0;
                    __syncthreads();
                    hw = 0;  // (wavefront 0's slice starts at x.pos and holds at least that candidate)
                }
                if (hw >= 0) {
                    const MiAhead &Hq = dh_mi_ahead[hw];
                    const int t = x.pos - Hq.pos0;
                    ev += computed;
                    if (Hq.stop[t]) {
                        stopped = true;
                        r_stat = Hq.stat[t];
                        r_p = Hq.pval[t];
                        r_pow = Hq.power[t];
                        nt = 1ull;
                    } else {  // significant: the job goes on at rank 1, seeded with its first test
                        best_p = Hq.pval[t];
                        best_stat = Hq.stat[t];
                        best_g = Hq.g[t];
                        best_df = Hq.df[t];
                        next = 1ull;
                    }
                }
            }
        }
        for (unsigned int step = 0u; !stopped && next < N && step < P.mi_team_steps; ++step) {
            ++n_rounds;
            const unsigned long long r0 = next + (unsigned long long)wave * per;
            unsigned long long r1 = r0 + per;
            if (r1 > N) r1 = N;
            FwSegOut o;
            const unsigned long long tq0 = MI_CLK();
            if (r0 < N) {
                const MiBest *seed = nullptr;
                if (best_p > 1e-290) {  // what the earlier rounds found: the tests it dominates skip their Q(a, x)
                    MiBest &sd = dh_mi_seed[wave];
                    sd.p = best_p;
                    sd.stat = best_stat;
                    sd.g = best_g;
                    sd.df = best_df;
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    seed = &sd;
                }
                o = mi_run_ranks_sel<L, NXY, PRE, R4>(T, cand, acc, a, P.max_k, P.max_tests, r0, r1, nullptr, 0, seed);
            } else {
                o.stop_rank = FW_RANK_NONE;
                o.stop_stat = o.stop_pval = 0.0;
                o.best_rank = 0ull;
                o.best_stat = 0.0;
                o.best_pval = -3.0;
                o.stop_df = o.stop_power = o.best_df = o.pad = 0;
                o.evaluated = 0ull;
            }
            if (lane == 0) dh_mi_trec[step & 1u][wave] = o;
            const unsigned long long tq1 = MI_CLK();
            __syncthreads();  // (two buffers: the records of round s are rewritten in round s + 2, behind the barrier of round s + 1)
#ifdef FW_MI_TICKS
            if (lane == 0) {
                atomicAdd(&Q->tm_run, tq1 - tq0);
                atomicAdd(&Q->tm_wait, MI_CLK() - tq1);
                atomicAdd(&Q->tm_steps, 1ull);
                atomicAdd(&Q->tm_tests, o.evaluated);
            }
#else
            (void)tq0;
            (void)tq1;
#endif
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const FwSegOut &q = dh_mi_trec[step & 1u][w];
                ev += q.evaluated;
                if (stopped) continue;
                if (q.stop_rank != FW_RANK_NONE) {
                    stopped = true;
                    r_stat = q.stop_stat;
                    r_p = q.stop_pval;
                    r_pow = q.stop_power;
                    nt = q.stop_rank + 1ull;
                } else if (q.best_pval >= 0.0 && q.best_pval >= best_p) {
                    best_p = q.best_pval;
                    best_stat = q.best_stat;
                    best_g = q.stop_stat;
                    best_df = q.best_df;
                }
            }
            next += 4ull * per;
            if (next > N) next = N;
        }
        const unsigned long long tk2 = MI_CLK();
        // ... the rest of a long enumeration: boards (the leader publishes and merges, all four work on the records)
        const bool tail = J.tail != 0;
        unsigned long long width = (unsigned long long)(tail ? P.mi_win0_tail : P.mi_win0);
        const unsigned long long chunk_min = tail ? P.mi_chunk_tail : P.mi_chunk_min;
        unsigned int bacc_off = MI_BACC_CAP;
        bool boarded = false;
        while (!stopped && next < N) {
            boarded = true;
            const unsigned long long W = (N - next) < width ? (N - next) : width;
            unsigned long long chunk = W / (unsigned long long)P.mi_chunk_div;
            chunk = chunk < chunk_min ? chunk_min : (chunk > P.mi_chunk_max ? P.mi_chunk_max : chunk);
            const unsigned int nch = (unsigned int)((W + chunk - 1ull) / chunk);
            if (wave == 0) {
                unsigned int bi, ro;
                const bool ok = mi_publish(Q, boards, bacc, bacc_off, acc, a, T, cand, next, W, chunk, nch, lane, bi, ro, best_p, best_g, best_df);
                if (!ok) {  // out of board space (never at the benchmark sizes): the leader carries on alone
                    const FwSegOut q = mi_run_ranks_sel<L, NXY, PRE, R4>(T, cand, acc, a, P.max_k, P.max_tests, next, next + W, nullptr, 0, nullptr);
                    if (lane == 0) {
                        J.mg.g = q.stop_stat;
                        J.mg.df = q.best_df;
                        J.mg.stop = q.stop_rank != FW_RANK_NONE;
                        J.mg.stat = J.mg.stop ? q.stop_stat : q.best_stat;
                        J.mg.p = J.mg.stop ? q.stop_pval : (q.best_pval < 0.0 ? -2.0 : q.best_pval);
                        J.mg.pow = q.stop_power;
                        J.mg.nt = q.stop_rank + 1ull;
                        J.mg.ev = q.evaluated;
                    }
                }
                if (lane == 0) J.board = ok ? bi : MI_BOARD_CAP;
            }
            __syncthreads();
            const unsigned int bi = J.board;
            if (bi < MI_BOARD_CAP) {
                MiBoard *b = boards + bi;
                while (mi_board_work<L, NXY, PRE, R4>(b, res, bacc, acc, lane)) {
                }
                if (wave == 0) {
                    MiWatch wd;
                    unsigned int dn = mi_ld_u32(&b->done);
                    mi_watch_begin(wd, dn);
                    while (dn < nch) {  // records claimed by other wavefronts: they are running
                        mi_nap_wait();
                        dn = mi_ld_u32(&b->done);
                        if (mi_watch_expired(wd, dn)) {
                            if (lane == 0) atomicExch(&Q->pad[0], 3u);
                            break;
                        }
                    }
                    const DhMerge mg = mi_merge(res, (long long)(unsigned int)(mi_ld_u64(&b->nr) >> 32), (int)nch, lane);
                    if (lane == 0) J.mg = mg;
                }
            }
            __syncthreads();
            const DhMerge mg = J.mg;
            ev += mg.ev;
            if (mg.stop) {
                stopped = true;
                r_stat = mg.stat;
                r_p = mg.p;
                r_pow = mg.pow;
                nt = mg.nt;
            } else if (mg.p != -2.0 && mg.p >= best_p) {
                best_p = mg.p;
                best_stat = mg.stat;
                best_g = mg.g;
                best_df = mg.df;
            }
            next += W;
            width *= 8ull;
        }
        if (!stopped) {  // every subset significant: the maximum-p result (tests.jl:338-345)
            r_stat = best_stat;
            r_p = best_p < 0.0 ? 0.0 : best_p;
            r_pow = 1;
            nt = N;
        }
        // The job's verdict changes the target state in LDS (dh_commit: x.pos, x.na, ...) and every wavefront reads that state while it
        // works on the job (x.pos, x.nc, x.phase, the whitelist, the look-ahead slot of x.pos): nobody may still be reading when the leader
        // commits.  r05 had this barrier BEHIND the commit only; a job that ended with a cached first test had no barrier at all between
        // its start and the commit, a late wavefront read the advanced x.pos, took another branch with a barrier of its own and stayed one
        // barrier behind (wrong records in its hands, one target's PC list differing about once in a thousand passes, or a hang).
        // Behind the commit the other wavefronts read nothing until the next job's first barrier, so this is the only one needed.
        __syncthreads();
        if (wave == 0) {
            const unsigned long long tk3 = MI_CLK();
            if (lane == 0) {
                x.r_first1 += (unsigned int)(tk2 - tk1);
                x.r_more1 += (unsigned int)(tk3 - tk2);
                if (boarded) x.c_eval_short += 1ull;
                x.c_eval_short += (unsigned long long)n_rounds << 32;  // (trace: lock-step rounds of the target in the high word)
            }
            x.c_ref += nt;
            x.c_calls += 1ull;
            x.c_eval += ev;
            x.c_alg += (P.max_k <= 3 && a <= FW_UNRANK32_A) ? dh_alg_bytes_disc32(a, ev, P.max_k, P.disc_bytes_per_col)
                                                            : dh_alg_bytes(a, ev, P.max_k, P.disc_bytes_per_col);
            if constexpr (TR) {
                if (stopped && !(r_p < P.alpha && r_pow)) mi_rej_record<L, NXY, PRE, R4>(Q, x, T, cand, acc, a, nt, r_stat, r_p, r_pow, lane);  // (wavefront 0 alone: the routine touches only its own wavefront's LDS slots, and the others wait at the next job's first barrier)
                dh_commit(x, A, lane, 1, r_stat, r_p, r_pow, P.alpha, P.elim_mode != 0);
            } else {
                dh_commit(x, A, lane, 1, r_stat, r_p, r_pow, P.alpha, EX);
            }
        }
    }
    if (wave == 0 && lane == 0) {
        x.r_more0 = (unsigned int)MI_CLK();
        tg[t] = x;
        atomicAdd(&Q->targets_done, 1u);
    }
    __syncthreads();
}

#ifdef FW_MI_TICKS
#define MI_TICK(slot, t0) do { if ((threadIdx.x & 63) == 0) dh_mi_ticks[threadIdx.x >> 6][slot] += wall_clock64() - (t0); } while (0)
#else
#define MI_TICK(slot, t0) do { (void)(t0); } while (0)
#endif
#ifndef DH_MI_OCC
#define DH_MI_OCC 1  // workgroups per CU the register budget is sized for
#endif
// EX: exact elimination (fw_learn_opts.elim_mode 1 / 2) -- a compile-time instantiation, so that the default one keeps its
// register allocation
// TR: the rejection log (fw_set_track_rejections) -- likewise; the tracking instantiation reads the elimination mode at run time
template <int L, int NXY, int PRE, bool R4, bool EX, bool TR>
__global__ __launch_bounds__(256, DH_MI_OCC) void dh_mi_target_kernel(DhTgt *__restrict__ tg, int ntg, const int32_t *__restrict__ order,
                                                           DhArrays A, MiDev M, DhParams P, MiQueue *__restrict__ Q,
                                                           MiBoard *__restrict__ boards, FwSegOut *__restrict__ res,
                                                           int32_t *__restrict__ bacc)
{
    const int lane = threadIdx.x & 63;
    // 100 MHz ticks per wavefront, summed into MiQueue at the end (FW_TRACE_HOST prints the averages): own first tests, board
    // phases (own records + waiting / helping), helping before jobs, the tail after the last target
    unsigned long long tk_seq = 0ull, tk_board = 0ull, tk_help = 0ull, tk_tail = 0ull;
#ifdef FW_MI_TICKS
    if (lane < 12) dh_mi_ticks[threadIdx.x >> 6][lane] = 0ull;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
#endif
    if (lane == 0) dh_mi_ahead[threadIdx.x >> 6].n = 0;  // (no look-ahead results yet)
    if (threadIdx.x == 0) {  // the launch context of the out-of-line routines (see DhMiCtx)
        dh_mi_ctx.A = A;
        dh_mi_ctx.M = M;
        dh_mi_ctx.P = P;
    }
    __syncthreads();
    const unsigned long long tk_begin = MI_CLK();
    // the heaviest targets (the first mi_team of the list): a workgroup each, all four wavefronts on it (dh_mi_team), taken in list
    // order by whichever workgroup is free; the list proper starts behind them
    for (;;) {
        if (threadIdx.x == 0) dh_mi_tj.go = (int)atomicAdd(&Q->next_team, 1u);
        __syncthreads();
        const unsigned int ts = (unsigned int)dh_mi_tj.go;
        __syncthreads();  // (dh_mi_team rewrites the descriptor)
        if (ts >= P.mi_team) break;
        dh_mi_team<L, NXY, PRE, R4, EX, TR>(tg, ntg, order[ts], Q, boards, res, bacc);
    }
    unsigned int jobctr = 0u;
    bool tail_seen = false;
    for (;;) {
        const unsigned int slot = P.mi_team + mi_wave_add(&Q->next_target, 1u, lane);
        if (slot >= (unsigned int)ntg) break;
        const int t = order[slot];
        // the target's state lives in LDS while its jobs run: every lane holds the same copy, and ~50 registers of it live across
        // the out-of-line test routine were part of what kept this kernel at one wavefront per SIMD
        DhTgt &x = dh_mi_x[threadIdx.x >> 6];
        if (lane == 0) {
            x = tg[t];
            if (A.wl_cnt) x.wl_n = (int32_t)A.wl_cnt[x.T];  // device-built whitelist: what the earlier launches of the schedule appended
            x.r_first0 = (unsigned int)MI_CLK();  // FW_TRACE_HOST: when the target was taken / finished (100 MHz ticks, low word)
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (;;) {
            const unsigned long long tka0 = MI_CLK();
            const bool more_jobs = dh_advance(x, A, lane, 1, (EX || TR) && P.elim_mode == 2);
            MI_TICK(6, tka0);
            if (!more_jobs) break;
            // other targets' big enumerations first: they are the critical path of the pass
            const unsigned long long tk0 = MI_CLK();
            // ... unless this target is one of the heavy ones: its own chain of jobs IS the critical path (cfg2 / cfg4: the
            // launch ended when the heaviest target did, 13 ms after the average wavefront had run out of targets)
            const bool heavy = P.mi_heavy > 0u && (unsigned int)x.nc >= P.mi_heavy;
            // the shared words (boards, target counters) are looked at before every FOURTH job: each look is two to four sc1 round
            // trips of ~2 us, and a chain of jobs that end with their first test (or cost nothing at all: mi_first4) paid more for
            // them than for its tests (cfg2 trace: 18.8 us per job against a 12 us test)
            const bool poll = (jobctr++ & 3u) == 0u;
            mi_u32x4 q4 = {0u, 0u, 0u, 0u};  // {next_target, targets_done, n_boards, hint}
            if (poll) q4 = mi_ld_u128(Q);
            if (P.mi_help_jobs && !heavy && poll && q4.z > q4.w)
                while (mi_help<L, NXY, PRE, R4>(Q, boards, res, bacc, lane) && mi_ld_u32(&Q->n_boards) > mi_ld_u32(&Q->hint)) {
                }
            const unsigned long long tk1 = MI_CLK();
            tk_help += tk1 - tk0;
            const int32_t *cands = x.phase == 0 ? A.cand0 + x.cand_off : A.tpc_key + x.co;
            const int32_t cand = cands[x.pos];
            const long long acc_off = DH_ACC_OFF(x, x.cur, 1);
            const int a = x.na;
            const unsigned long long N = dh_enum_size(a, P.max_k, P.max_tests);
            // the first tests: alone.  Elimination-phase jobs nearly always run to the end (the member passed every test against
            // almost this pool a moment ago): a big one goes to a board at once, whole enumeration in one window
            const bool elim_full = x.phase == 1 && P.mi_elim_min > 0u && N > (unsigned long long)P.mi_elim_min;
            // the owner's sequential prefix.  While every wavefront still has targets of its own, boards cost more than they give
            // (a prefix of 4 instead of 16: 55 -> 72 ms at cfg4 on one GPU); once the target list is exhausted the idle wavefronts
            // do nothing but poll, and the chains of the last heavy targets ARE the rest of the pass: hand over after mi_seq_tail
            // tests (one rank of eight, cfg4: 46.9 -> 37.2 ms of conditional stage)
            // (tail: no target left to claim AND fewer than one wavefront in eight still owns one -- cfg2 has as many targets as
            // the launch has wavefronts: "list exhausted" alone switched every job of the pass to the short prefix, 15 -> 22 ms)
            if (poll) tail_seen = q4.x + P.mi_team >= (unsigned int)ntg && ((unsigned int)ntg - q4.y) * 8u <= gridDim.x * 4u;
            const bool tail = tail_seen;
            const unsigned long long seq = tail ? P.mi_seq_tail : (heavy ? P.mi_seq_heavy : P.mi_seq);
            unsigned long long next = elim_full ? 0ull : (N < seq ? N : seq);
            MI_TICK(7, tk1);
            FwSegOut o;
            bool first_known = false;
            if constexpr (R4) {
                MiAhead &H = dh_mi_ahead[threadIdx.x >> 6];
                if (P.mi_ahead && x.phase == 0 && a >= 1 && next >= 1ull) {
                    bool hit = H.T == x.T && H.na == a && x.pos >= H.pos0 && x.pos < H.pos0 + H.n;
                    unsigned long long computed = 0ull;
                    if (!hit && x.nc - x.pos >= 2) {
                        const int nb = x.nc - x.pos < 4 ? x.nc - x.pos : 4;
                        mi_first4<L>(x.T, x.pos, cands + x.pos, nb, A.acc + acc_off, a, P.max_k, P.max_tests);
                        computed = (unsigned long long)H.n;
                        hit = true;
                    }
                    if (hit) {
                        const int t = x.pos - H.pos0;
                        first_known = true;
                        o.stop_rank = FW_RANK_NONE;
                        o.stop_stat = o.stop_pval = 0.0;
                        o.best_rank = 0ull;
                        o.best_stat = 0.0;
                        o.best_pval = -3.0;
                        o.stop_df = o.stop_power = o.best_df = o.pad = 0;
                        o.evaluated = 0ull;
                        if (H.stop[t]) {
                            o.stop_rank = 0ull;
                            o.stop_stat = H.stat[t];
                            o.stop_pval = H.pval[t];
                            o.stop_df = H.df[t];
                            o.stop_power = H.power[t];
                        } else {
                            if (next > 1ull) {  // ranks 1 .. of this candidate's own job, seeded with its first test
                                MiBest &sd = dh_mi_seed[threadIdx.x >> 6];
                                if (lane == 0) {
                                    sd.p = H.pval[t];
                                    sd.stat = H.stat[t];
                                    sd.g = H.g[t];
                                    sd.df = H.df[t];
                                }
                                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                                __builtin_amdgcn_wave_barrier();
                                o = mi_run_ranks_sel<L, NXY, PRE, R4>(x.T, cand, A.acc + acc_off, a, P.max_k, P.max_tests, 1ull, next, nullptr, 0,
                                                                      H.pval[t] > 1e-290 ? &sd : nullptr);
                            }
                            if (o.stop_rank == FW_RANK_NONE && !(o.best_pval >= H.pval[t])) {  // the first test is still the maximum
                                o.best_pval = H.pval[t];
                                o.best_stat = H.stat[t];
                                o.best_df = H.df[t];
                                o.stop_stat = H.g[t];
                            }
                        }
                        o.evaluated += computed;
                    }
                }
            }
            if (!first_known)
                o = mi_run_ranks_sel<L, NXY, PRE, R4>(x.T, cand, A.acc + acc_off, a, P.max_k, P.max_tests, 0ull, next, nullptr, 0, nullptr);
            unsigned long long ev = o.evaluated, nt = 0ull;
            bool stopped = o.stop_rank != FW_RANK_NONE;
            double r_stat = stopped ? o.stop_stat : 0.0, r_p = stopped ? o.stop_pval : 0.0;
            int r_pow = stopped ? o.stop_power : 1;
            double best_p = o.best_pval, best_stat = o.best_stat, best_g = stopped ? 0.0 : o.stop_stat;  // (+ G^2, df: the seed of the boards)
            int best_df = o.best_df;
            if (stopped) nt = o.stop_rank + 1ull;
            // (in the tail the records are short and the first window wide: the wavefronts that poll outnumber the records of a window)
            unsigned long long width = elim_full ? N : (unsigned long long)(tail ? P.mi_win0_tail : P.mi_win0);
            const unsigned long long chunk_min = tail ? P.mi_chunk_tail : P.mi_chunk_min;
            unsigned int bacc_off = MI_BACC_CAP;  // this job's write-through copy of its accepted list (made with its first board)
            const unsigned long long tk2 = MI_CLK();
            tk_seq += tk2 - tk1;
            if (lane == 0) x.r_first1 += (unsigned int)(tk2 - tk1);  // FW_TRACE_HOST: this target's ticks in sequential prefixes / board phases
            while (!stopped && next < N) {
                const unsigned long long W = (N - next) < width ? (N - next) : width;
                unsigned long long chunk = W / (unsigned long long)P.mi_chunk_div;
                chunk = chunk < chunk_min ? chunk_min : (chunk > P.mi_chunk_max ? P.mi_chunk_max : chunk);
                const unsigned int nch = (unsigned int)((W + chunk - 1ull) / chunk);
                unsigned int bi, ro;
                const unsigned long long tkp0 = MI_CLK();
                const bool published = mi_publish(Q, boards, bacc, bacc_off, A.acc + acc_off, a, x.T, cand, next, W, chunk, nch, lane, bi, ro,
                                                  best_p, best_g, best_df);
                MI_TICK(9, tkp0);
                DhMerge mg;
                if (!published) {  // out of board space (never at the benchmark sizes): the owner carries on alone
                    const FwSegOut q = mi_run_ranks_sel<L, NXY, PRE, R4>(x.T, cand, A.acc + acc_off, a, P.max_k, P.max_tests, next, next + W, nullptr, 0, nullptr);
                    mg.stop = q.stop_rank != FW_RANK_NONE;
                    mg.stat = mg.stop ? q.stop_stat : q.best_stat;
                    mg.p = mg.stop ? q.stop_pval : (q.best_pval < 0.0 ? -2.0 : q.best_pval);
                    mg.pow = q.stop_power;
                    mg.nt = q.stop_rank + 1ull;
                    mg.ev = q.evaluated;
                    mg.g = q.stop_stat;
                    mg.df = q.best_df;
                } else {
                    MiBoard *b = boards + bi;
                    while (mi_board_work<L, NXY, PRE, R4>(b, res, bacc, A.acc + acc_off, lane)) {
                    }
                    MiWatch wd;
                    unsigned int dn = mi_ld_u32(&b->done);
                    mi_watch_begin(wd, dn);
                    while (dn < nch) {  // records claimed by other wavefronts: they are running
                        if (heavy || !mi_help<L, NXY, PRE, R4>(Q, boards, res, bacc, lane)) {
                            const unsigned long long tkw0 = MI_CLK();
                            mi_nap_wait();
                            MI_TICK(10, tkw0);
                            if (mi_watch_expired(wd, mi_ld_u32(&b->done))) {  // 2 s without a record finishing: a logic error, not a workload -- report instead of hanging the GPU
                                if (lane == 0) atomicExch(&Q->pad[0], 1u);
                                break;
                            }
                        } else {
                            mi_watch_begin(wd, dn);  // (helped another board meanwhile: the clock starts again)
                        }
                        dn = mi_ld_u32(&b->done);
                    }
                    const unsigned long long tkm0 = MI_CLK();
                    mg = mi_merge(res, (long long)ro, (int)nch, lane);
                    MI_TICK(11, tkm0);
                }
                ev += mg.ev;
                if (mg.stop) {
                    stopped = true;
                    r_stat = mg.stat;
                    r_p = mg.p;
                    r_pow = mg.pow;
                    nt = mg.nt;
                } else if (mg.p != -2.0 && mg.p >= best_p) {
                    best_p = mg.p;
                    best_stat = mg.stat;
                    best_g = mg.g;
                    best_df = mg.df;
                }
                next += W;
                width *= 8ull;
            }
            {
                const unsigned long long tk3 = MI_CLK();
                tk_board += tk3 - tk2;
                if (lane == 0) {
                    x.r_more1 += (unsigned int)(tk3 - tk2);
                    if (next > (elim_full ? 0ull : (N < seq ? N : seq))) x.c_eval_short += 1ull;  // jobs that went to a board
                }
            }
            if (!stopped) {  // every subset significant: the maximum-p result (tests.jl:338-345)
                r_stat = best_stat;
                r_p = best_p < 0.0 ? 0.0 : best_p;
                r_pow = 1;
                nt = N;
            }
            const unsigned long long tkc0 = MI_CLK();
            x.c_ref += nt;
            x.c_calls += 1ull;
            x.c_eval += ev;
            x.c_alg += (P.max_k <= 3 && a <= FW_UNRANK32_A) ? dh_alg_bytes_disc32(a, ev, P.max_k, P.disc_bytes_per_col)
                                                            : dh_alg_bytes(a, ev, P.max_k, P.disc_bytes_per_col);
            if constexpr (TR) {
                if (stopped && !(r_p < P.alpha && r_pow)) mi_rej_record<L, NXY, PRE, R4>(Q, x, x.T, cand, A.acc + acc_off, a, nt, r_stat, r_p, r_pow, lane);
                dh_commit(x, A, lane, 1, r_stat, r_p, r_pow, P.alpha, P.elim_mode != 0);
            } else {
                dh_commit(x, A, lane, 1, r_stat, r_p, r_pow, P.alpha, EX);
            }
            MI_TICK(8, tkc0);
        }
        if (lane == 0) {
            x.r_more0 = (unsigned int)MI_CLK();
            tg[t] = x;
            atomicAdd(&Q->targets_done, 1u);  // (a termination count, not a hand-off: the host reads tg after the kernel)
        }
    }
    // no targets left to start: work on boards until every target has finished
    const unsigned long long tk_t0 = MI_CLK();
    MiWatch wd;  // progress of the launch as seen from here: a target finished or a board was opened (both counters only grow)
    mi_watch_begin(wd, 0u);
    unsigned int wd_periods = 0u;
    while (mi_ld_u32(&Q->targets_done) < (unsigned int)ntg && mi_ld_u32(&Q->pad[0]) == 0u) {
        if (!mi_help<L, NXY, PRE, R4>(Q, boards, res, bacc, lane)) {
            mi_nap_tail();
            wd.n |= 255u;  // (a nap is ~7 us: look at the clock every time)
            if (mi_watch_expired(wd, mi_ld_u32(&Q->targets_done) + mi_ld_u32(&Q->n_boards))) {
                wd.t0 = 0ull;
                if (++wd_periods >= 5u) {  // 10 s in which no target finished and no board was opened
                    if (lane == 0) atomicExch(&Q->pad[0], 2u);
                    break;
                }
            }
        } else {
            wd_periods = 0u;
            wd.t0 = 0ull;
        }
    }
    tk_tail = MI_CLK() - tk_t0;
    if (lane == 0) {  // t_body: first tests of own jobs, t_ctl: board phases, t_sleep: helping before jobs, n_seg: tail; total in pad[1] units of 2^10 ticks
        atomicAdd(&Q->t_body, tk_seq);
        atomicAdd(&Q->t_ctl, tk_board);
        atomicAdd(&Q->t_sleep, tk_help);
        atomicAdd(&Q->n_seg, tk_tail);
        atomicAdd(&Q->t_total, tk_t0 - tk_begin);
#ifdef FW_MI_TICKS
        for (int q = 0; q < 12; ++q) atomicAdd(&Q->tick[q], dh_mi_ticks[threadIdx.x >> 6][q]);
#endif
    }
}

// One wavefront per target: the lanes merge the job's segment records in parallel, then run the sequential part
// (commit, advance, next job) in lock-step -- every lane holds the same copy of the state, lane 0 writes.
//
// Elimination-phase look-ahead (spec_depth > 0, FW_ELIM_FULL windows): the phase tests the members c_0, c_1, ... of TPC one
// after the other, each against the pool without itself, and nearly always keeps them (cfg3: 96 %), so a target with
// 170 members is a chain of 170 rounds of one job each.  With the job of c_0 (pool L_0) the launch therefore also
// carries the jobs of c_1 .. c_d against the pools they will see IF every earlier member is kept:
// L_{j+1} = (L_j + [c_j]) \ {c_{j+1}} (hiton.jl:134-149: a kept member re-enters the pool at its end), each in its own
// accepted-list buffer.  The step kernel commits them in order; the first dropped member ends the chain (the later
// look-ahead jobs saw a pool that still held it: their results are discarded and they run again).
template <bool TR>
__device__ __forceinline__ void dh_step_dev(DhTgt *__restrict__ tg, int ntg, DhGlobal *__restrict__ g, const DhArrays &A,
                                            const FwSegOut *__restrict__ so, const long long *__restrict__ seg0,
                                            unsigned long long *__restrict__ win, unsigned int *__restrict__ sp,
                                            unsigned long long *__restrict__ win2, const int32_t *__restrict__ act, const DhParams &P,
                                            const int ci /* position in the list of unfinished targets (seg0 is indexed by it) */)
{
    const int lane = threadIdx.x & 63;
    const int d1 = P.spec_depth + 1;
    unsigned long long mywin = 0ull;
    if (ci < (int)g->n_act) {
        const int t = act[(size_t)g->act_sel * ntg + ci];
        DhTgt x = tg[t];
        const long long jseg0 = seg0[ci];
        const int nsp_done = x.nsp;
        const int spmode_done = x.spmode;
        // records of the target's own job, then of each look-ahead job (their window jwin2 can differ from the job's)
        const int nseg_all = (int)(seg0[ci + 1] - jseg0);
        int jnseg = nseg_all / (1 + nsp_done), jnseg2 = jnseg;
        if (nsp_done > 0 && spmode_done == 1) {
            const unsigned long long sl = g->seglen;  // the finished launch's segment length (the next plan has not run yet)
            jnseg = (int)dh_ceil_div(x.jwin, sl, 1.0 / (double)sl);
            jnseg2 = (nseg_all - jnseg) / nsp_done;
        }
        x.nsp = 0;
        x.spmode = 0;
        bool finished = false, kept = false;
        if (x.jactive) {
            if (x.phase == 0) (x.jnext == 0ull ? x.r_first0 : x.r_more0) += 1u;
            else (x.jnext == 0ull ? x.r_first1 : x.r_more1) += 1u;
            const DhMerge M = dh_merge<TR>(so, jseg0, jnseg, lane);
            double r_stat = 0.0, r_p = 1.0;
            int r_pow = 0;
            [[maybe_unused]] int r_df = 0;
            unsigned long long r_nt = 0ull;
            bool done = false;
            if (M.stop) {
                if constexpr (TR) r_df = M.df;
                r_stat = M.stat;
                r_p = M.p;
                r_pow = M.pow;
                r_nt = M.nt;
                done = true;
            } else if (M.p != -2.0 && M.p >= x.jbest_p) {
                x.jbest_p = M.p;
                x.jbest_stat = M.stat;
            }
            x.jevaluated += M.ev;
            if (!done) {
                x.jnext += x.jwin;
                const unsigned long long growth = g->launched_ranks < P.small_launch ? P.growth_small : (g->n_live_prev > P.busy_jobs ? P.growth_busy : P.growth);
                x.jwidth *= growth;
                if (x.jnext >= x.jN) {
                    r_stat = x.jbest_stat;
                    r_p = x.jbest_p < 0.0 ? 0.0 : x.jbest_p;
                    r_pow = 1;
                    r_nt = x.jN;
                    done = true;
                }
            }
            if (done) {
                x.jactive = 0;
                finished = true;
                x.c_ref += r_nt;
                x.c_calls += 1ull;
                x.c_eval += x.jevaluated;
                x.c_eval_short += x.na <= FW_HK_A ? x.jevaluated : 0ull;
                x.na_max = x.na > x.na_max ? x.na : x.na_max;
                x.c_alg += dh_alg_bytes(x.na, x.jevaluated, P.max_k, P.disc_bytes_per_col);
                if constexpr (TR) kept = dh_commit<true>(x, A, lane, d1, r_stat, r_p, r_pow, P.alpha, P.elim_mode != 0, P.max_k, r_nt, r_df);
                else kept = dh_commit(x, A, lane, d1, r_stat, r_p, r_pow, P.alpha, P.elim_mode != 0);
            }
        }
        if (nsp_done > 0) {
            // look-ahead jobs, committed in candidate order while the assumption they were built on holds: elimination
            // phase -- every earlier member kept (own pool buffers, whole enumerations); interleaving phase -- every
            // earlier candidate dropped (same accepted list, first window only: a candidate that survives its first
            // window becomes the target's job and ends the chain)
            // ... interleaving phase, spmode 1 (the job was in its LAST window, i.e. it had survived its first one and was about
            // to be accepted): first windows of the next candidates against accepted + [candidate]; they count if the candidate
            // was indeed accepted, and then follow the same in-order rule
            const bool ph1 = x.phase == 1, acc_mode = spmode_done == 1;
            const int n = acc_mode ? x.na : x.na - (kept ? 1 : 0), cur0 = x.cur;
            const unsigned long long wsp = acc_mode ? x.jwin2 : x.jwin;  // look-ahead jobs ride with the first window of the target's job
            if (acc_mode) x.jN = x.jN2;  // the enumeration the look-ahead jobs belong to (accepted list one entry longer)
            bool valid = finished && ((ph1 || acc_mode) ? kept : !kept);
            for (int j = 1; j <= nsp_done; ++j) {
                const DhMerge M = dh_merge<TR>(so, jseg0 + (long long)jnseg + (long long)(j - 1) * jnseg2, jnseg2, lane);
                if (!valid) {  // built on an assumption that failed: executed for nothing
                    x.c_eval += M.ev;
                    continue;
                }
                if (ph1) {
                    x.cur = (cur0 + j) % d1;
                    x.na = n;
                }
                if (!M.stop && wsp < x.jN) {  // interleaving: survived the first window -> continues as the target's job
                    const unsigned long long growth = g->launched_ranks < P.small_launch ? P.growth_small : (g->n_live_prev > P.busy_jobs ? P.growth_busy : P.growth);
                    x.jactive = 1;
                    x.jnext = wsp;
                    x.jwidth = wsp * growth;
                    x.jbest_p = M.p != -2.0 ? M.p : -1.0;
                    x.jbest_stat = M.p != -2.0 ? M.stat : 0.0;
                    x.jevaluated = M.ev;
                    valid = false;
                    continue;
                }
                const double r_stat = M.stop ? M.stat : (M.p != -2.0 ? M.stat : 0.0);
                const double r_p = M.stop ? M.p : (M.p < 0.0 ? 0.0 : M.p);
                x.c_ref += M.stop ? M.nt : x.jN;
                x.c_calls += 1ull;
                x.c_eval += M.ev;
                x.c_eval_short += n <= FW_HK_A ? M.ev : 0ull;
                x.c_alg += dh_alg_bytes(n, M.ev, P.max_k, P.disc_bytes_per_col);
                bool k;
                if constexpr (TR) k = dh_commit<true>(x, A, lane, d1, r_stat, r_p, M.stop ? M.pow : 1, P.alpha, P.elim_mode != 0, P.max_k, M.nt, M.df);
                else k = dh_commit(x, A, lane, d1, r_stat, r_p, M.stop ? M.pow : 1, P.alpha, P.elim_mode != 0);
                valid = ph1 ? k : !k;
            }
        }
        if (!x.jactive && x.phase != 2 && dh_advance(x, A, lane, d1, P.elim_mode == 2)) {
            const unsigned long long N = dh_enum_size(x.na, P.max_k, P.max_tests);  // (32-bit binomials where every term fits)
            x.jN = N;
            x.jnext = 0ull;
            // Elimination phase: the candidate passed every test against (almost) this pool a moment ago, so nearly all
            // of these jobs run to the end -- evaluate the whole enumeration in one window instead of two rounds
            // (FW_ELIM_FULL=0 disables; cfg3: -20 % rounds for +2 % evaluated tests)
            x.jwidth = (x.phase == 1 && P.elim_full) ? N : (x.na >= 64 ? P.w0_big : P.w0_small);
            x.jbest_p = -1.0;
            x.jbest_stat = 0.0;
            x.jevaluated = 0ull;
            x.jactive = 1;
            if (lane == 0 && (unsigned int)x.na > g->max_a) atomicMax(&g->max_a, (unsigned int)x.na);  // rare: only on a new maximum
            {   // phase 0: the list can still take every whitelisted neighbour it has not met; phase 1: pools never exceed TPC (plus the
                // second entries of whitelisted members) -- in exact mode as well: its pools are those of fast mode when every member is kept
                const int abi = x.phase == 0 ? x.na + x.wl_n - x.wl_used : (x.na > x.ntpc ? x.na : x.ntpc);
                if (lane == 0 && (unsigned int)abi > g->max_ab) atomicMax(&g->max_ab, (unsigned int)abi);
            }
            if (x.phase == 0 && P.spec0_depth > 0 && g->launched_ranks < P.spec0_below && g->n_live_prev < P.spec0_jobs) {
                const int32_t *cands = A.cand0 + x.cand_off;
                int q = 0;
                // (light launches -- the first feed-forward rounds, a rank of a multi-GPU job: the tests are nearly free, the dependent
                // rounds are the cost -> more candidates per round)
                const int depth = g->launched_ranks < P.spec0_light_below ? P.spec0_depth_light : P.spec0_depth;
                while (q < depth && x.pos + 1 + q < x.nc) {
                    if (x.wl_n > 0 && dh_in_wl(x, A, cands[x.pos + 1 + q])) break;  // whitelisted: joins without a test
                    ++q;
                }
                x.nsp = q;
            }
            if (x.phase == 1 && P.elim_full && P.spec_depth > 0 && g->launched_ranks < P.spec_below) {
                // pools of the next members (see above), all built in ONE pass over the current pool:
                // L_j = (L_0 without c_1 .. c_j, in L_0's order) + [c_0, ..., c_{j-1}]
                const int32_t *cands = A.tpc_key + x.co;
                const int n = x.na;
                const int32_t c0 = cands[x.pos];
                int32_t cn[DH_MAX_SPEC];
                int Q = 0;
#pragma unroll
                for (int j = 0; j < DH_MAX_SPEC; ++j) {
                    cn[j] = -1;
                    if (j == Q && j < P.spec_depth && x.pos + 1 + j < x.nc) {
                        const int32_t c = cands[x.pos + 1 + j];
                        if (!(x.wl_n > 0 && dh_in_wl(x, A, c))) {  // whitelisted: kept without a test (hiton.jl:20-30)
                            cn[j] = c;
                            Q = j + 1;
                        }
                    }
                }
                const int32_t *src = A.acc + DH_ACC_OFF(x, x.cur, d1);
                int w[DH_MAX_SPEC];
#pragma unroll
                for (int j = 0; j < DH_MAX_SPEC; ++j) w[j] = 0;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                for (int base = 0; base < n; base += 64) {
                    const int i = base + lane;
                    const int32_t v = i < n ? src[i] : -1;
                    bool alive = i < n;
#pragma unroll
                    for (int j = 0; j < DH_MAX_SPEC; ++j) {
                        if (j < Q) {  // wavefront-uniform
                            alive = alive && v != cn[j];
                            const unsigned long long m = __ballot(alive);
                            int32_t *dst = A.acc + DH_ACC_OFF(x, (x.cur + 1 + j) % d1, d1);
                            if (alive) dst[w[j] + __popcll(m & ((1ull << lane) - 1ull))] = v;
                            w[j] += __popcll(m);
                        }
                    }
                }
                int q = 0;
#pragma unroll
                for (int j = 0; j < DH_MAX_SPEC; ++j) {
                    // a pool that lost anything but exactly c_1 .. c_{j+1} (duplicated entries: whitelists) ends the chain
                    if (j == q && j < Q && w[j] == n - (j + 1)) {
                        int32_t *dst = A.acc + DH_ACC_OFF(x, (x.cur + 1 + j) % d1, d1);
                        if (lane <= j) {
                            int32_t tail = c0;
#pragma unroll
                            for (int u = 0; u < DH_MAX_SPEC; ++u)
                                if (lane == u + 1) tail = cn[u];
                            dst[w[j] + lane] = tail;
                        }
                        q = j + 1;
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
                x.nsp = q;
            }
        }
        if (x.jactive) {
            const unsigned long long left = x.jN - x.jnext;
            mywin = x.jwidth < left ? x.jwidth : left;
        }
        x.jwin = mywin;
        if (x.nsp > 0) x.jwin2 = mywin, x.jN2 = x.jN;  // spmode 0: the look-ahead jobs share the job's window
        if (x.jactive && x.phase == 0 && x.jnext > 0ull && mywin == x.jN - x.jnext && x.nsp == 0 && P.spec1_depth > 0 &&
            g->launched_ranks < P.spec0_below && g->n_live_prev < P.spec0_jobs) {
            // The candidate survived its first window(s) and this launch finishes its enumeration: it is about to be accepted
            // (cfg3: a heavy target accepts half of its candidates, and each of them cost a first window, a last window and only
            // then the next candidate -- the longest chain of the pass).  The first windows of the next candidates ride along
            // against accepted + [candidate]: the entry is written behind the list now (dh_commit writes the same value there)
            const int32_t *cands = A.cand0 + x.cand_off;
            int q = 0;
            while (q < P.spec1_depth && x.pos + 1 + q < x.nc) {
                if (x.wl_n > 0 && dh_in_wl(x, A, cands[x.pos + 1 + q])) break;  // whitelisted: joins without a test
                ++q;
            }
            if (q > 0) {
                if (lane == 0) A.acc[DH_ACC_OFF(x, x.cur, d1) + x.na] = cands[x.pos];
                const unsigned long long N2 = dh_enum_size(x.na + 1, P.max_k, P.max_tests);
                const unsigned long long w0 = x.na + 1 >= 64 ? P.w0_big : P.w0_small;
                x.nsp = q;
                x.spmode = 1;
                x.jN2 = N2;
                x.jwin2 = w0 < N2 ? w0 : N2;
                if (lane == 0 && (unsigned int)(x.na + 1) > g->max_a) atomicMax(&g->max_a, (unsigned int)(x.na + 1));
            }
        }
        if (lane == 0) {
            tg[t] = x;
            win[t] = mywin;  // 0 = no job in the coming launch
            sp[t] = (unsigned int)x.nsp;
            win2[t] = x.nsp > 0 ? x.jwin2 : 0ull;
        }
    }
}

template <bool TR>
__global__ __launch_bounds__(256) void dh_step_kernel(DhTgt *__restrict__ tg, int ntg, DhGlobal *__restrict__ g, DhArrays A,
                                                      const FwSegOut *__restrict__ so, const long long *__restrict__ seg0,
                                                      unsigned long long *__restrict__ win, unsigned int *__restrict__ sp,
                                                      unsigned long long *__restrict__ win2, const int32_t *__restrict__ act, DhParams P)
{
    dh_step_dev<TR>(tg, ntg, g, A, so, seg0, win, sp, win2, act, P, (int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
}

// one workgroup: totals of the coming launch, its segment length, per-target segment counts and their exclusive scan.
// The segment length has no upper cap here, so the launch never holds more than seg_target + (live jobs) segments:
// the fixed grid (seg_target + targets) always covers it.
#define DH_PER 16  // targets per planning thread held in registers (more targets: extra passes over global memory)
struct DhPlanArgs {
    unsigned int seg_target, seg_q, seg_min, log_cap;
    ulonglong2 *log;
    unsigned long long seg_a, seg_b;
};
// NT = threads of the one workgroup that plans (1024: dh_plan_kernel)
// (the last workgroup of dh_step_kernel)
template <int NT>
__device__ __forceinline__ void dh_plan_dev(int ntg, DhGlobal *__restrict__ g, const unsigned long long *__restrict__ win,
                                            const unsigned int *__restrict__ sp, const unsigned long long *__restrict__ win2,
                                            const int32_t *__restrict__ act_all, long long *__restrict__ seg0, const DhPlanArgs PA)
{
    constexpr int NW = NT / 64;
    const unsigned int seg_target = PA.seg_target, seg_q = PA.seg_q, seg_min = PA.seg_min, log_cap = PA.log_cap;
    ulonglong2 *__restrict__ log = PA.log;
    const unsigned long long seg_a = PA.seg_a, seg_b = PA.seg_b;
    __shared__ unsigned long long s_tot[16];
    __shared__ unsigned int s_live[16], s_wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int na = (int)g->n_act;  // unfinished targets; everything below is indexed by the position in that list
    const int32_t *act = act_all + (size_t)g->act_sel * ntg;
    const int per = (na + NT - 1) / NT;
    const int b = tid * per, e = (b + per) < na ? (b + per) : na;
    unsigned long long tot = 0ull;
    unsigned int live = 0u;
    unsigned long long wr[DH_PER];   // this thread's windows (registers when per <= DH_PER)
    unsigned long long w2r[DH_PER];  // window of each look-ahead job (win2: equal to the job's own except in spmode 1)
    unsigned int mr[DH_PER];         // look-ahead jobs
#pragma unroll
    for (int q = 0; q < DH_PER; ++q) {
        const int tq = (b + q < e) ? act[b + q] : 0;
        wr[q] = (b + q < e) ? win[tq] : 0ull;
        mr[q] = (b + q < e) ? sp[tq] : 0u;
        w2r[q] = (b + q < e && mr[q] > 0u) ? win2[tq] : 0ull;
    }
#pragma unroll
    for (int q = 0; q < DH_PER; ++q) {
        tot += wr[q] + w2r[q] * mr[q];
        live += wr[q] != 0ull ? 1u + mr[q] : 0u;
    }
    for (int t = b + DH_PER; t < e; ++t) {
        const unsigned long long w = win[act[t]];
        const unsigned int m = sp[act[t]];
        tot += w + (m ? win2[act[t]] * m : 0ull);
        live += w != 0ull ? 1u + m : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tot += __shfl_xor(tot, o);
        live += __shfl_xor(live, o);
    }
    if (lane == 0) {
        s_tot[wave] = tot;
        s_live[wave] = live;
    }
    __syncthreads();
    unsigned long long total = 0ull;
    unsigned int n_live = 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        total += s_tot[w];
        n_live += s_live[w];
    }
    // small launches: fewer, longer segments (one / two residency waves of workgroups instead of three) -- every
    // workgroup pays its set-up (accepted list, thresholds, LDS table) once, and a launch of a few M ranks is latency-bound
    const unsigned int tgt = total < seg_a ? (seg_target + 2u) / 3u : (total < seg_b ? (2u * seg_target + 2u) / 3u : seg_target);
    unsigned long long seglen = (total / tgt + seg_q - 1ull) / seg_q * seg_q;
    seglen = seglen < seg_min ? seg_min : seglen;
    const double inv = 1.0 / (double)seglen;
    unsigned int local = 0u;
    unsigned int nr[DH_PER];
#pragma unroll
    for (int q = 0; q < DH_PER; ++q) {
        nr[q] = dh_ceil_div(wr[q], seglen, inv) + dh_ceil_div(w2r[q], seglen, inv) * mr[q];
        local += nr[q];
    }
    for (int t = b + DH_PER; t < e; ++t)
        local += dh_ceil_div(win[act[t]], seglen, inv) + (sp[act[t]] ? dh_ceil_div(win2[act[t]], seglen, inv) * sp[act[t]] : 0u);
    unsigned int incl = local;  // inclusive scan inside the wavefront, then over the 16 wavefront totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    unsigned int wbase = 0u, ns = 0u;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        if (w < wave) wbase += s_wsum[w];
        ns += s_wsum[w];
    }
    unsigned int run = wbase + incl - local;
#pragma unroll
    for (int q = 0; q < DH_PER; ++q)
        if (b + q < e) {
            seg0[b + q] = (long long)run;
            run += nr[q];
        }
    for (int t = b + DH_PER; t < e; ++t) {
        seg0[t] = (long long)run;
        run += dh_ceil_div(win[act[t]], seglen, inv) + (sp[act[t]] ? dh_ceil_div(win2[act[t]], seglen, inv) * sp[act[t]] : 0u);
    }
    if (tid == 0) {
        seg0[na] = (long long)ns;
        g->ns = ns;
        g->any_big = 0u;
        g->seglen = (unsigned int)seglen;
        g->launched_ranks = total;
        g->n_live_prev = n_live;
        if (n_live == 0u) g->done = 1u;
        const unsigned int r = g->rounds;
        g->ns_ring[r & 63u] = ns;
        g->rounds = r + 1u;
        if (log && r < log_cap) log[r] = make_ulonglong2(total, ((unsigned long long)n_live << 32) | ns);  // FW_DH_LOG
    }
}

__global__ __launch_bounds__(1024) void dh_plan_kernel(int ntg, DhGlobal *__restrict__ g, const unsigned long long *__restrict__ win,
                                                       const unsigned int *__restrict__ sp, const unsigned long long *__restrict__ win2,
                                                       const int32_t *__restrict__ act_all, long long *__restrict__ seg0, DhPlanArgs PA)
{
    dh_plan_dev<1024>(ntg, g, win, sp, win2, act_all, seg0, PA);
}
// The same plan on ONE wavefront per SIMD (r06).  The 1 024-thread form is 4 wavefronts x 127 registers per SIMD: it starts only on a CU that is EMPTY, and while the
// other chain's long-list segment kernel (3 x 168 registers per SIMD, thousands of workgroups pending) keeps every CU refilled that happens when that kernel has
// nothing left to dispatch -- cfg5: 3.1 ms per call, 7 588 calls (profiles/r05_cfg5_kernel_stats.csv; stream priority does not help: r06_cfg5_plan_kernel.txt).
// 256 threads fit beside two resident segment wavefronts as soon as one workgroup leaves.  cfg5 59.1 -> 57.8 s; and at cfg3, whose size-3 kernel fills the register
// file with 4 x 128, the two chains stop holding each other's rounds up: plan 27 -> 8 us per call in the two-chain pass, headline 159.6 -> 152.2 ms
// (profiles/r06_cfg5_plan_kernel.txt, r06_cfg3_plan_kernel.txt).  This 256-thread form is the default (FW_DH_PLAN_SMALL=0: the 1 024-thread form).
__global__ __launch_bounds__(256) void dh_plan_small_kernel(int ntg, DhGlobal *__restrict__ g, const unsigned long long *__restrict__ win,
                                                            const unsigned int *__restrict__ sp, const unsigned long long *__restrict__ win2,
                                                            const int32_t *__restrict__ act_all, long long *__restrict__ seg0, DhPlanArgs PA)
{
    dh_plan_dev<256>(ntg, g, win, sp, win2, act_all, seg0, PA);
}

// fz rounds (r06): the local correlation matrix of every target that has one -- M[a][b] = cor[id(a)][id(b)], id(0) = T, id(1 ..) = T's
// level-0 neighbours in ascending id order (every variable a job of T can name: candidates, TPC / PC members and whitelisted
// neighbours are all level-0 neighbours of T).  The size-3 test gathers one matrix entry cor[z3][z2] per test, 64 scattered 4-byte
// words per wavefront step out of a 400 MB matrix: L2 hit 88 %, i.e. every step waited for a fabric round trip and the pass read
// 105 GB through the fabric (profiles/r05_cfg3_pmc_summary.json) -- out of a target's own (deg + 1)^2 floats (cfg3's heaviest: 250 KB)
// the same gathers stay in L2.  One workgroup per target, rows a, columns b over the threads.
__global__ __launch_bounds__(256) void dh_tmat_build_kernel(const DhTgt *__restrict__ tg, int ntg, const int32_t *__restrict__ nb_idx,
                                                            const float *__restrict__ cor, int p, float *__restrict__ tmat)
{
    __shared__ int32_t s_id[4096];
    const DhTgt &x = tg[blockIdx.x];
    if (x.tm_off < 0) return;  // (workgroup-uniform)
    const int m = x.nb_n + 1;
    const int32_t *ids = nb_idx + x.nb_off;
    for (int b = threadIdx.x; b < m; b += 256) s_id[b] = b == 0 ? x.T : ids[b - 1];
    __syncthreads();
    float *M = tmat + x.tm_off;
    // rows blockIdx.y, blockIdx.y + gridDim.y, ...: four rows in flight per thread (independent gathers)
    for (int a0 = (int)blockIdx.y * 4; a0 < m; a0 += (int)gridDim.y * 4)
        for (int b = threadIdx.x; b < m; b += 256) {
            const size_t col = (size_t)s_id[b];
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = a0 + q < m ? cor[(size_t)s_id[a0 + q] * (size_t)p + col] : 0.0f;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (a0 + q < m) M[(size_t)(a0 + q) * m + b] = v[q];
        }
}

// The record of ranks [start, end) of target x's job on candidate Y against the list of acc_len entries at acc_off: what the segment
// body reads about a job, the target's local matrix included where it has one (dh_fill_one, dh_fz_light_kernel)
__device__ __forceinline__ FwSeg dh_seg_record(const DhTgt &x, const DhArrays &A, int32_t Y, long long acc_off, int acc_len, int32_t pad,
                                               unsigned long long start, unsigned long long end)
{
    FwSeg sg;
    sg.X = x.T;
    sg.Y = Y;
    sg.acc_off = acc_off;
    sg.acc_len = acc_len;
    sg.pad = pad;
    sg.start = start;
    sg.end = end;
    const bool has_tm = A.tmat != nullptr && x.tm_off >= 0;
    sg.tm = has_tm ? (uint64_t)(A.tmat + x.tm_off) : 0ull;
    sg.tm_ids = has_tm ? (uint64_t)(A.nb_idx + x.nb_off) : 0ull;
    sg.tm_m = has_tm ? x.nb_n + 1 : 0;
    sg.pad1 = 0;
    return sg;
}

// segment record s of the coming launch (one thread)
__device__ __forceinline__ void dh_fill_one(const unsigned int s, const DhTgt *__restrict__ tg, int ntg, DhGlobal *__restrict__ g,
                                            const long long *__restrict__ seg0, const DhArrays &A, FwSeg *__restrict__ segs, int d1,
                                            const int32_t *__restrict__ act)
{
    int lo = 0, hi = (int)g->n_act;  // first list position with seg0 > s; the job owning slot s is the one before it
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg0[mid] <= (long long)s)
            lo = mid + 1;
        else
            hi = mid;
    }
    const DhTgt &x = tg[act[(size_t)g->act_sel * ntg + lo - 1]];
    const unsigned long long seglen = g->seglen;
    unsigned long long k = (unsigned long long)((long long)s - seg0[lo - 1]);
    const int32_t *cands = x.phase == 0 ? A.cand0 + x.cand_off : A.tpc_key + x.co;
    unsigned int slot = 0;  // 0 = the target's job, j = its j-th look-ahead job (own window jwin2; elimination: own pool buffer)
    if (x.nsp > 0) {
        const unsigned int all = (unsigned int)(seg0[lo] - seg0[lo - 1]);
        const unsigned int n0 = x.spmode == 1 ? dh_ceil_div(x.jwin, seglen, 1.0 / (double)seglen) : all / (1u + (unsigned int)x.nsp);
        if ((unsigned int)k >= n0) {
            const unsigned int per = (all - n0) / (unsigned int)x.nsp;
            slot = 1u + ((unsigned int)k - n0) / per;
            k -= (unsigned long long)n0 + (unsigned long long)(slot - 1u) * per;
        }
    }
    const bool acc_mode = slot > 0u && x.spmode == 1;  // list = accepted + [current candidate], first window of its own enumeration
    const int acc_len = x.na + (acc_mode ? 1 : 0);
    if (acc_len > FW_TAB_A) g->any_big = 1u;  // same value from every writer
    const unsigned long long lo_r = acc_mode ? 0ull : x.jnext;
    const unsigned long long start = lo_r + k * seglen;
    const unsigned long long hi_r = lo_r + (slot > 0u ? x.jwin2 : x.jwin);
    // (pad -- fz_nz: the job's record slot = the target's index in the run, dh_nz_recs_kernel)
    segs[s] = dh_seg_record(x, A, cands[x.pos + (int)slot], DH_ACC_OFF(x, x.phase == 1 ? (x.cur + (int)slot) % d1 : x.cur, d1), acc_len,
                            act[(size_t)g->act_sel * ntg + lo - 1], start, start + seglen < hi_r ? start + seglen : hi_r);
}
__global__ __launch_bounds__(256) void dh_fill_kernel(const DhTgt *__restrict__ tg, int ntg, DhGlobal *__restrict__ g,
                                                      const long long *__restrict__ seg0, const DhArrays A,
                                                      FwSeg *__restrict__ segs, int d1, const int32_t *__restrict__ act)
{
    const unsigned int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= g->ns) return;
    dh_fill_one(s, tg, ntg, g, seg0, A, segs, d1, act);
}

// (r04 fused step + plan (+ fill) into the last workgroup to finish, r05 into a cooperative grid with one device-memory barrier and a
// redundant plan in every workgroup: both bit-identical, neither faster -- the barrier and the second plan cost what the saved
// launches cost, ~5 us of idle time per device-wide dependency either way.  profiles/r04_fused_round.json, profiles/r05_coop_round.json.)

// One workgroup, once per batch of rounds (between dh_step_kernel and dh_plan_kernel): drops the finished targets from
// the list the three kernels above walk.  Most targets finish early (cfg3: 10 000 targets, a few hundred alive for
// most of the rounds; cfg4: 50 020 / a few thousand), so step, plan and fill shrink with the work that is left.
// Order-preserving; writes the other half of the ping-pong list and flips act_sel.
__global__ __launch_bounds__(1024) void dh_compact_kernel(const DhTgt *__restrict__ tg, int ntg, DhGlobal *__restrict__ g,
                                                          int32_t *__restrict__ act_all)
{
    __shared__ unsigned int s_wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int na = (int)g->n_act;
    const unsigned int sel = g->act_sel;
    const int32_t *src = act_all + (size_t)sel * ntg;
    int32_t *dst = act_all + (size_t)(sel ^ 1u) * ntg;
    const int per = (na + 1023) / 1024;
    const int b = tid * per, e = (b + per) < na ? (b + per) : na;
    unsigned int local = 0u;
    for (int i = b; i < e; ++i) {
        const DhTgt &x = tg[src[i]];
        local += (x.phase != 2 || x.jactive) ? 1u : 0u;
    }
    unsigned int incl = local;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned int v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
    if (lane == 63) s_wsum[wave] = incl;
    __syncthreads();
    unsigned int wbase = 0u, total = 0u;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        if (w < wave) wbase += s_wsum[w];
        total += s_wsum[w];
    }
    unsigned int pos = wbase + incl - local;
    for (int i = b; i < e; ++i) {
        const int t = src[i];
        const DhTgt &x = tg[t];
        if (x.phase != 2 || x.jactive) dst[pos++] = t;
    }
    if (tid == 0) {
        g->n_act = total;
        g->act_sel = sel ^ 1u;
    }
}

// fz_nz on the device rounds (r05): the per-job records of the sub-matrix kernel (fznz_submat_kernel: correlations over the rows where
// T and the candidate are both non-zero, statfuns.jl:138-155), one slot per target.  A job that enters its FIRST window gets a fresh
// record -- variables, list, the target's own arena slice ((candidates + 2)^2 floats: a list never outgrows the candidate list) -- and
// its matrix is computed in this round; a job in a later window keeps record and matrix (bit 0 of pad: nothing to compute), as does
// a target without a job.  (The host pool recomputes the matrix for every window of a job.)
__global__ __launch_bounds__(256) void dh_nz_recs_kernel(const DhTgt *__restrict__ tg, int ntg, const DhGlobal *__restrict__ g,
                                                         const int32_t *__restrict__ act, const DhArrays A, FwNzJob *__restrict__ recs,
                                                         const long long *__restrict__ arena_off)
{
    const int ci = (int)(blockIdx.x * 256u + threadIdx.x);
    if (ci >= (int)g->n_act) return;
    const int t = act[(size_t)g->act_sel * ntg + ci];
    const DhTgt &x = tg[t];
    FwNzJob *r = recs + t;
    if (x.jactive && x.jwin > 0ull && x.jnext == 0ull) {
        r->X = x.T;
        r->Y = (x.phase == 0 ? A.cand0 + x.cand_off : A.tpc_key + x.co)[x.pos];
        r->acc_off = DH_ACC_OFF(x, x.cur, 1);
        r->acc_len = x.na;
        r->m = x.na + 2;
        r->cor_off = arena_off[t];
        r->pad = 0;
    } else {
        r->pad = 1;
    }
}

// ---- light Fisher-z targets: one resident workgroup per target, no device rounds ---------------------------------------------------
// A target with a handful of level-0 neighbours is a chain of a few dozen jobs of a few hundred tests each; through the rounds above
// every link of that chain costs a device-wide dependency (segment kernel -> step -> plan -> fill), ~50 us for work that fills a
// fraction of one workgroup (cfg3: nine of the ten feed-forward rounds, 21-25 dependent rounds each).  Targets of a round are
// independent and such a target's longest enumeration is shorter than one segment, so here a workgroup runs its target's whole HITON-PC
// in the reference's own order -- no window, no look-ahead, no other workgroup to wait for -- the way dh_mi_target_kernel runs the
// discrete kinds.  Wave 0 is the state machine of dh_step_dev (dh_advance, dh_commit, the same per-target counters); all four
// wavefronts run a job as ONE segment [0, N) through the segment kernel's own body, so statistic, p-value, first stop and the "later
// wins ties" maximum are those of the rounds bit for bit.  The host decides which targets are light (dh_is_light, from static sizes);
// the others leave at once and go through DhRounds afterwards.
__host__ __device__ inline bool dh_is_light(int deg, int cap, int light_deg) { return light_deg > 0 && deg <= light_deg && cap <= light_deg; }

__shared__ DhTgt dh_lt_x;    // the workgroup's target between two jobs
__shared__ FwSeg dh_lt_seg;  // the job all four wavefronts run next
__shared__ int dh_lt_go;     // ... 0: none (the target has finished, or hit one of the bounds below and stays unfinished)

__global__ __launch_bounds__(256, 4) void dh_fz_light_kernel(DhTgt *__restrict__ tg, int ntg, int light_deg, const DhArrays A,
                                                             FwSegOut *__restrict__ so, const DhParams P, const float *__restrict__ cor, int p,
                                                             double zscale, const double *__restrict__ thr)
{
    const int t = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63;
    if (t >= ntg || !dh_is_light(tg[t].nb_n, tg[t].cap, light_deg)) return;  // (workgroup-uniform)
    const int d1 = P.spec_depth + 1;
    // every job consumes an interleaving candidate (at most cap) or a member of TPC (at most one per candidate): a hard bound on the
    // loop.  A target that would pass it, or whose list would not fit the table variant, is left unfinished: the rounds take it
    // up where a slot has any, and the host reports unfinished targets as FW_ERR_DEVICE (dh_download, dh_sched_finish)
    const int job_max = 2 * tg[t].cap;
    for (int job = 0;; ++job) {
        if (tid < 64) {  // wave 0, all lanes in lock-step as in dh_step_dev
            DhTgt x = job == 0 ? tg[t] : dh_lt_x;
            if (job > 0) {  // the finished job: one record, one window (dh_step_dev's commit of a whole enumeration)
                const DhMerge M = dh_merge(so, (long long)t, 1, lane);
                const double r_stat = M.stop ? M.stat : (M.p != -2.0 ? M.stat : 0.0);
                const double r_p = M.stop ? M.p : (M.p < 0.0 ? 0.0 : M.p);
                (x.phase == 0 ? x.r_first0 : x.r_first1) += 1u;
                x.c_ref += M.stop ? M.nt : x.jN;
                x.c_calls += 1ull;
                x.c_eval += M.ev;
                x.c_eval_short += x.na <= FW_HK_A ? M.ev : 0ull;
                x.na_max = x.na > x.na_max ? x.na : x.na_max;
                x.c_alg += dh_alg_bytes(x.na, M.ev, P.max_k, P.disc_bytes_per_col);
                dh_commit(x, A, lane, d1, r_stat, r_p, M.stop ? M.pow : 1, P.alpha, P.elim_mode != 0);
            }
            bool go = x.phase != 2 && dh_advance(x, A, lane, d1, P.elim_mode == 2);
            go = go && job < job_max && x.na <= FW_TAB_A;
            if (go) x.jN = dh_enum_size(x.na, P.max_k, P.max_tests);
            if (lane == 0) {
                dh_lt_x = x;
                dh_lt_go = go ? 1 : 0;
                if (go)
                    dh_lt_seg = dh_seg_record(x, A, (x.phase == 0 ? A.cand0 + x.cand_off : A.tpc_key + x.co)[x.pos], DH_ACC_OFF(x, x.cur, d1),
                                              x.na, t, 0ull, x.jN);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the list wave 0 wrote, the record in LDS
        __syncthreads();
        if (!dh_lt_go) break;
        FwSeg sg = dh_lt_seg;  // (the body takes a workgroup-uniform record: out of LDS it is, but the compiler has to be told)
        sg.X = __builtin_amdgcn_readfirstlane(sg.X);
        sg.Y = __builtin_amdgcn_readfirstlane(sg.Y);
        sg.acc_off = (int64_t)mi_rfl64((unsigned long long)sg.acc_off);
        sg.acc_len = __builtin_amdgcn_readfirstlane(sg.acc_len);
        sg.pad = __builtin_amdgcn_readfirstlane(sg.pad);
        sg.start = mi_rfl64(sg.start);
        sg.end = mi_rfl64(sg.end);
        sg.tm = mi_rfl64(sg.tm);
        sg.tm_ids = mi_rfl64(sg.tm_ids);
        sg.tm_m = __builtin_amdgcn_readfirstlane(sg.tm_m);
        fz_seg_body<false, false, true>(cor, p, sg, A.acc + sg.acc_off, false, so + t, P.max_k, P.alpha, zscale, P.max_tests, thr,
                                        (const FwNzJob *)nullptr, 0ll);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the record, whichever thread wrote it
        __syncthreads();
    }
    if (tid == 0) tg[t] = dh_lt_x;
}

// ---- the whole feed-forward schedule on the device (fwi_devhiton_mi_schedule, fwi_devhiton_fz_schedule) ------------------------------
// per-target state of EVERY target of the schedule, built on the device from the level-0 CSR: a target's arrays (candidates in
// hiton.jl:211-217 order, TPC / PC, accepted lists, whitelist) all sit at its level-0 offset nb_off[T] with its degree as capacity --
// what dh_build_targets makes on the host.  tgt_T: the targets in the order of tg (discrete: schedule order; Fisher-z: slot order =
// round, chain, index in the chain).  levels (discrete kinds, else null): a constant variable has nothing to test.  slot_tm (Fisher-z,
// else null): the offsets of the local correlation matrices (dh_tm_off); absent, tm_off stays what the memset gives.  wl_unsorted:
// 1 where the whitelists are read as the appends left them (discrete), 0 where the round that reads them sorts them first
// (dh_fz_round_begin_kernel)
__global__ __launch_bounds__(256) void dh_sched_init_kernel(DhTgt *__restrict__ tg, int nt, const int32_t *__restrict__ tgt_T,
                                                            const long long *__restrict__ nb_off, const int32_t *__restrict__ levels,
                                                            const long long *__restrict__ slot_tm, int wl_unsorted)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= nt) return;
    DhTgt x;
    __builtin_memset(&x, 0, sizeof(x));
    const int T = tgt_T[i];
    const long long o = nb_off[T];
    const int deg = (int)(nb_off[T + 1] - o);
    x.T = T;
    x.nc = x.cap = deg;
    x.phase = (deg == 0 || (levels && levels[T] < 2)) ? 2 : 0;  // hiton.jl:182-184 (a constant variable), :336-338 (no candidate)
    x.co = x.cand_off = x.wl_off = x.nb_off = o;
    x.nb_n = deg;
    x.wl_unsorted = wl_unsorted;
    if (slot_tm) x.tm_off = slot_tm[i];
    tg[i] = x;
}

// after a round: the running graph of interleaved.jl:136-140, kept only where a later round will read it -- target T with u in PC(T)
// is a whitelisted neighbour of u (hiton.jl:20-30) when u's own round comes later; T's own list is never read again.  One entry per
// (T, u): no duplicates.  The level-0 lists are symmetric and PC(T) is a subset of T's candidates, so u's list holds at most deg(u).
__global__ __launch_bounds__(256) void dh_wl_append_kernel(const DhTgt *__restrict__ tg, int ntg, const int32_t *__restrict__ pc_key,
                                                           const int32_t *__restrict__ round_of, int round, int32_t *__restrict__ wl,
                                                           const long long *__restrict__ nb_off, unsigned int *__restrict__ wl_cnt)
{
    const int t = (int)(blockIdx.x * 4u + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (t >= ntg) return;
    const int T = tg[t].T, npc = tg[t].npc;
    const long long co = tg[t].co;
    for (int i = lane; i < npc; i += 64) {
        const int32_t u = pc_key[co + i];
        if (round_of[u] > round) wl[nb_off[u] + (long long)atomicAdd(&wl_cnt[u], 1u)] = T;
    }
}

// the list of unfinished targets at the start of a round of targets: every target, in order
__global__ __launch_bounds__(256) void dh_iota_kernel(int32_t *__restrict__ act, int n)
{
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i < n) act[i] = i;
}

// Start of a chain's round of targets (one workgroup per target): the whitelist that the earlier rounds appended (dh_wl_append_kernel)
// is sorted in place -- its entries are distinct, so an entry's rank is the number of smaller ones -- which gives dh_in_wl the early
// exit it has on the host-built lists.  The rank sort is quadratic in the list and stages it in 16 KB of LDS: choose_path keeps runs
// with a level-0 list beyond 4096 entries on the round loop, so the unsorted flag below is never set by the schedule (it keeps the
// kernel correct should that gate move); the round's control state is what
// dh_upload writes: every target on the list, no segment, a zeroed record.  wl_max: the longest whitelist of the chain's round (the
// host reads this word before it enqueues the round's first batch: DhRounds::enqueue_batch, any_big).
__global__ __launch_bounds__(256) void dh_fz_round_begin_kernel(DhTgt *__restrict__ tg, int ntg, const unsigned int *__restrict__ wl_cnt,
                                                                int32_t *__restrict__ wl, DhGlobal *__restrict__ g, long long *__restrict__ seg0,
                                                                int32_t *__restrict__ act, unsigned int *__restrict__ wl_max)
{
    __shared__ int32_t s_w[4096];
    const int t = (int)blockIdx.x, tid = (int)threadIdx.x;
    if (t >= ntg) return;
    DhTgt &x = tg[t];
    const int n = (int)wl_cnt[x.T];  // (workgroup-uniform; at most the degree: dh_wl_append_kernel)
    if (n > 1 && n <= 4096) {
        int32_t *w = wl + x.wl_off;
        for (int i = tid; i < n; i += 256) s_w[i] = w[i];
        __syncthreads();
        for (int i = tid; i < n; i += 256) {
            const int32_t e = s_w[i];
            int r = 0;
            for (int j = 0; j < n; ++j) r += s_w[j] < e;
            w[r] = e;
        }
    }
    if (tid == 0) {
        x.wl_n = n;
        x.wl_unsorted = n > 4096;
        act[t] = t;
        seg0[t] = 0;
        if (n > 0) atomicMax(wl_max, (unsigned int)n);
    }
    if (t == 0) {
        unsigned int *gw = (unsigned int *)g;
        for (int i = tid; i < (int)(sizeof(DhGlobal) / 4); i += 256) gw[i] = 0u;
        __syncthreads();
        if (tid == 0) {
            g->n_act = (unsigned int)ntg;
            seg0[ntg] = 0;
        }
    }
}

// results of the whole schedule, packed for ONE small download: every target's PC entries (target, neighbour, statistic, p) as a block
// of consecutive records in insertion order -- the blocks land where an atomic ticket puts them: the host's CSR over targets
// (fw_hiton.cpp: a stable counting sort by target) does not depend on the order of the blocks -- and the per-target counters summed
// (integers and multiples of 1/8: every order gives the same sums).  tot[0] entries, [1] tests in reference order, [2] jobs,
// [3] executed tests, [4] unfinished targets (must stay 0); alg: algorithmic bytes
__global__ __launch_bounds__(256) void dh_sched_pack_kernel(const DhTgt *__restrict__ tg, int nt, const int32_t *__restrict__ pc_key,
                                                         const double *__restrict__ pc_stat, const double *__restrict__ pc_p,
                                                         int32_t *__restrict__ o_t, int32_t *__restrict__ o_u, double *__restrict__ o_s,
                                                         double *__restrict__ o_p, unsigned long long *__restrict__ tot, double *__restrict__ alg)
{
    // (one set of atomics per target, six on one line for each of cfg3's 10 000 targets, was 0.6 ms per pass: the totals are taken by
    // one thread per target and reduced per wavefront first -- one ticket and one set of atomics per 64 targets)
    __shared__ unsigned long long s_base[256];
    const int tid = (int)threadIdx.x, lane = tid & 63, t = (int)blockIdx.x * 256 + tid;
    unsigned long long npc = 0ull, ref = 0ull, calls = 0ull, ev = 0ull, unfinished = 0ull;
    double al = 0.0;
    if (t < nt) {
        const DhTgt &x = tg[t];
        npc = (unsigned long long)x.npc;
        ref = x.c_ref;
        calls = x.c_calls;
        ev = x.c_eval;
        unfinished = x.phase != 2 ? 1ull : 0ull;
        al = x.c_alg;
    }
    unsigned long long incl = npc;  // entries of the wavefront's targets up to and including this one
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long v = __shfl_up(incl, o);
        if (lane >= o) incl += v;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ref += __shfl_xor(ref, o);
        calls += __shfl_xor(calls, o);
        ev += __shfl_xor(ev, o);
        unfinished += __shfl_xor(unfinished, o);
        al += __shfl_xor(al, o);
    }
    unsigned long long wbase = 0ull;
    if (lane == 63) {
        if (incl) wbase = atomicAdd(&tot[0], incl);
        if (ref) atomicAdd(&tot[1], ref);
        if (calls) atomicAdd(&tot[2], calls);
        if (ev) atomicAdd(&tot[3], ev);
        if (unfinished) atomicAdd(&tot[4], unfinished);
        if (al != 0.0) atomicAdd(alg, al);
    }
    s_base[tid] = __shfl(wbase, 63) + incl - npc;
    __syncthreads();
    // the lists as before: a wavefront per target, here the 64 targets of its own totals one after the other
    for (int j = 0; j < 64; ++j) {
        const int u = tid - lane + j, tu = (int)blockIdx.x * 256 + u;
        if (tu >= nt) break;
        const DhTgt &x = tg[tu];
        const unsigned long long base = s_base[u];
        const int n = x.npc;
        for (int i = lane; i < n; i += 64) {
            o_t[base + i] = x.T;
            o_u[base + i] = pc_key[x.co + i];
            o_s[base + i] = pc_stat[x.co + i];
            o_p[base + i] = pc_p[x.co + i];
        }
    }
}

}  // namespace

// ---- host side ----

static std::mutex dh_cnt_mu;  // concurrent chains share the context's counters

// A device arena described ONCE: the layout function runs twice over the same code -- without a base pointer it only adds up the
// size (every take() returns nullptr), with one it hands out the buffers.  Every buffer starts on a 256-byte boundary.
struct DhArena {
    char *base = nullptr;
    size_t used = 0;
    template <class T>
    T *take(size_t count, size_t extra_bytes = 0)
    {
        T *q = base ? (T *)(base + used) : nullptr;
        used += (sizeof(T) * count + extra_bytes + 255) & ~(size_t)255;
        return q;
    }
};
template <class Bufs, class Sizes>
static int dh_arena_reserve(fw_ctx *c, FwDevBuf &b, Bufs (*layout)(DhArena &, const Sizes &), const Sizes &z, Bufs *out)
{
    DhArena sizing;
    layout(sizing, z);
    if (int rc = fw_dev_reserve(c, b, sizing.used)) return rc;
    DhArena a{(char *)b.ptr};
    *out = layout(a, z);
    assert(a.used == sizing.used);
    return FW_OK;
}

// timing events (+ end-of-batch events without timing) of one call: the destructor synchronises the stream and destroys them on EVERY
// exit path (error returns and the watchdog of the persistent kernel included: r02 leaked 66 events per failed call and left the
// stream running)
struct DhEvents {
    hipStream_t st;
    std::vector<hipEvent_t> ev, ev_end;
    bool ok = true;
    DhEvents(hipStream_t s, int n_timing, int n_end) : st(s), ev((size_t)n_timing, nullptr), ev_end((size_t)n_end, nullptr)
    {
        for (hipEvent_t &e : ev) ok = ok && hipEventCreate(&e) == hipSuccess;
        for (hipEvent_t &e : ev_end) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    }
    ~DhEvents()
    {
        (void)hipStreamSynchronize(st);
        for (hipEvent_t &e : ev)
            if (e) (void)hipEventDestroy(e);
        for (hipEvent_t &e : ev_end)
            if (e) (void)hipEventDestroy(e);
    }
};

// window / look-ahead / board policy of a run (the sweeps that chose the defaults are quoted where each value is set; every knob is
// read per call)
static DhParams dh_make_params(fw_ctx *c, int ntg, int spec_depth, int spec0_depth)
{
    DhParams P{};
    P.alpha = c->P.alpha;
    P.max_k = c->P.max_k;
    P.max_tests = c->P.max_tests;
    P.small_launch = fw_small_launch();
    P.elim_full = fw_knob_int(knob::FW_ELIM_FULL, 1);
    P.growth_small = fw_knob_pos(knob::FW_DH_GROWTH_SMALL, 256ull);
    P.growth = fw_knob_pos(knob::FW_DH_GROWTH, 4ull);  // cfg3 sweeps: r01 4 -> 322 ms, 8 -> 321.5, 16 -> 331, 32 -> 350; r02 (three chains) 2 -> 219.6, 4 -> 218.3, 8 -> 219.7, 16 -> 241 (the host pool uses 16: its rounds cost 3x more)
    P.growth_busy = fw_knob_pos(knob::FW_DH_GROWTH_BUSY, 4ull);
    P.busy_jobs = (unsigned int)fw_knob_pos(knob::FW_DH_BUSY_JOBS, 2048ull);
    P.spec_depth = spec_depth;
    P.spec_below = fw_knob_pos(knob::FW_DH_SPEC_BELOW, (c->P.max_k <= 3 && ntg >= 256) ? 30000000ull : 12000000ull);  // chains of few targets (a rank of 4 / 8: 98 / 49 per chain) are latency-bound and pay for it: slowest of 8 ranks 83.9 -> 91.0 ms with 30 M;  // max_k 4-5: whole enumerations of the look-ahead pools are too dear in big launches (cfg5, first 40 000 targets: 0.97 -> 1.95 s with 30 M)  // (r03, after the job-count gate of the interleaving look-ahead moved: 12 M -> 199.8 ms, 20 M 193.6, 30 M 193.4, 50 M 194.7, none 193.6; cfg3 without feed-forward 172.1 -> 168.4)
    P.spec0_depth = spec0_depth;
    P.spec0_below = fw_knob_pos(knob::FW_DH_SPEC0_BELOW, 12000000ull);
    P.spec0_depth_light = spec0_depth > 0 ? std::min(std::max(fw_knob_int(knob::FW_DH_SPEC0_LIGHT, spec0_depth), spec0_depth), DH_MAX_SPEC) : 0;
    P.spec0_light_below = fw_knob_pos(knob::FW_DH_SPEC0_LIGHT_BELOW, 400000ull);
    P.spec0_jobs = (unsigned int)fw_knob_pos(knob::FW_DH_SPEC0_JOBS, 4096ull);  // (r03: 512 kept it off in the light feed-forward rounds of 1 024 targets: cfg3 204.8 -> 198.6 ms, 9 222 -> 7 966 launches)
    // look-ahead behind a candidate that is about to be accepted (dh_step_kernel, spmode 1)
    P.spec1_depth = c->P.kind == FW_FZ ? std::min(std::max(fw_knob_int(knob::FW_DH_SPEC1, 2), 0), DH_MAX_SPEC) : 0;
    P.mi_seq = (unsigned int)fw_knob_pos(knob::FW_MI_SEQ, 48ull);  // r04 sweep on the final kernels (cfg4, ms with / without feed-forward, two runs each): 8: 149 / 106, 16 (r02-r03): 111.0 / 72.5, 24: 118 / 71.8, 32: 102.4 / 70.9, 48: 102.4 / 70.5, 64: 102.2 / 70.8, 128: 112.9 / 72.6, never a board: 111.5 / 79.1; cfg2 neutral
    P.mi_win0 = (unsigned int)fw_knob_pos(knob::FW_MI_WIN0, 128ull);
    P.mi_chunk_div = (unsigned int)fw_knob_pos(knob::FW_MI_CHUNK_DIV, 256ull);
    P.mi_chunk_min = (unsigned int)fw_knob_pos(knob::FW_MI_CHUNK_MIN, 8ull);
    P.mi_chunk_max = (unsigned int)fw_knob_pos(knob::FW_MI_CHUNK_MAX, 64ull);
    P.mi_help_jobs = (unsigned int)fw_knob_int(knob::FW_MI_HELP_JOBS, 1);
    P.mi_elim_min = (unsigned int)fw_knob_int(knob::FW_MI_ELIM_MIN, 64);
    P.mi_heavy = (unsigned int)fw_knob_int(knob::FW_MI_HEAVY, 48);
    P.mi_seq_heavy = (unsigned int)fw_knob_int(knob::FW_MI_SEQ_HEAVY, (int)P.mi_seq);
    P.mi_seq_tail = (unsigned int)fw_knob_int(knob::FW_MI_SEQ_TAIL, 4);
    P.mi_ahead = (unsigned int)fw_knob_int(knob::FW_MI_AHEAD, 1);
    P.mi_chunk_tail = (unsigned int)std::max(1, fw_knob_int(knob::FW_MI_CHUNK_TAIL, (int)P.mi_chunk_min));
    P.mi_win0_tail = (unsigned int)std::max(1, fw_knob_int(knob::FW_MI_WIN0_TAIL, 1024));
    const bool fz = c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ;  // (fz_nz: the same segment kernels on job-local matrices)
    // first window of an interleaving-phase job with fewer than 64 accepted variables.  r04 sweep at cfg3 (two chains, look-ahead 4 / 2,
    // growth 4; ms per pass / launches): 64: 198.7 / 9 790, 128: 194.8, 256 (r01-r03): 189.1 / 8 090, 512: 186.3, 1 024: 183.9, 2 048: 184.7,
    // 4 096: 182.5 / 7 194, 8 192: 184.3, 16 384: 187.6 -- the executed tests move by less than 1 % over that range (a job that stops does
    // so within its first wavefront steps whatever the window), the launches by 25 %.  max_k > 3 keeps 256 (not measured at full cfg5 size).
    // Second sweep (first window 4 096): first window of jobs with 64 accepted variables or more 8 192: 191.2, 16 384 (r01-r03): 183.8,
    // 24 576: 182.4, 32 768: 178.1 - 179.9, 49 152: 182.4, 65 536: 191.4; with 32 768 the small window 2 048: 177.3, 4 096: 178.1, 8 192: 181.7.
    // (FW_W0_SMALL, FW_W0_BIG: fz only; r04 sweep: DESIGN section 4)
    P.w0_small = fz ? fw_knob_pos(knob::FW_W0_SMALL, c->P.max_k <= 3 ? 2048ull : 256ull) : 16ull;
    P.w0_big = fz ? fw_knob_u64(knob::FW_W0_BIG, c->P.max_k <= 3 ? 32768ull : 16384ull) : 16ull;
    P.seg_q = fz ? 256u : 4u;
    P.seg_min = fz ? 256u : 8u;
    P.disc_bytes_per_col = fz ? 0.0 : (double)c->P.n * (c->P.kind == FW_MI ? 1.0 : 2.0) / 8.0;
    P.elim_mode = c->elim_mode;
    return P;
}

// launch policy of one call of fwi_devhiton_run: derived from (kind, max_k, ntg, elim_mode) and the knobs, which are latched at the
// first call
struct DhPolicy {
    bool nzk;         // fz_nz (r05): rounds like fz, with the sub-matrix kernel in front of the segment kernel
    bool fz;          // the rounds over the Fisher-z segment kernels (fz_nz: on job-local matrices)
    bool per_target;  // discrete kinds: one persistent launch (dh_mi_target_kernel) instead of rounds
    bool use_hp, plan_small;
    unsigned seg_target, grid_seg;
    unsigned long long seg_a, seg_b;
    int spec_depth, spec0_depth;
    int nb;          // rounds per batch
    int time_every;  // one segment launch in this many is timed
    int tm_min;      // smallest degree of a target that gets a local correlation matrix (0: none)
    const char *log_path;
};
constexpr int DH_BATCH = 16;
constexpr unsigned DH_LOG_CAP = 1u << 16;

static DhPolicy dh_policy(const fw_ctx *c, int ntg)
{
    DhPolicy y{};
    const bool fz_kind = c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ;
    // fz rounds (r06): local correlation matrices for the targets whose jobs can be long (dh_tmat_build_kernel); FW_FZ_TMAT=0: none
    static const int tm_env = fw_knob_int(knob::FW_FZ_TMAT, -1);            // smallest degree that gets one (0: off)
    y.tm_min = tm_env >= 0 ? tm_env : (c->P.max_k > 3 ? 1 : 16);  // (cfg3 sweep: 16; cfg5: 1 -- 54.6 -> 53.8 s)
    static const unsigned seg_target_env = (unsigned)fw_seg_target();
    y.seg_target = seg_target_env ? seg_target_env : (fz_kind ? (c->P.max_k > 3 ? 8192u : 3072u) : 4096u);  // cfg3 sweep: 3072; cfg5 (max_k 5, launches of 10^8 ranks and more): 8192 (r06: 53.9 -> 52.4 s)
    // elimination-phase look-ahead (fz, FW_ELIM_FULL windows; see dh_step_kernel): FW_DH_SPEC = members tested ahead per
    // target, FW_DH_SPEC_BELOW = only while the last launch held fewer ranks than this.  cfg3 sweep (ms per pass, one
    // GPU / one rank of 8): off 326.7 / 112.0; depth 4 always 338 / 103; depth 4 below 4M 318.5 / 104.4, below 8M
    // 317.3 / 104.6, below 12M 314.8 / 103.6, below 16M 341 -- a launch that already fills the GPU only pays for the
    // jobs wasted behind every dropped member (3.7 % of the members at cfg3)
    // Exact elimination (elim_mode 1 / 2): no look-ahead job is ever discarded (a rejected member re-enters the pool as well), so
    // the chain of a target with m members takes about m / (depth + 1) rounds; default DH_SPEC_EXACT
    static const int spec_env = fw_knob_int(knob::FW_DH_SPEC, -1);
    const int spec_dflt = c->elim_mode != 0 ? DH_SPEC_EXACT : 4;
    y.spec_depth = c->P.kind == FW_FZ ? std::min(std::max(spec_env >= 0 ? spec_env : spec_dflt, 0), DH_MAX_SPEC) : 0;
    // discrete kinds: persistent wavefronts + boards (dh_mi_target_kernel); FW_MI_ROUNDS=1 keeps the level-synchronous rounds over
    // the segment kernels (the path of the ABI's fw_test_subsets_batch) for comparison.  Fisher-z always runs as rounds (a
    // persistent-workgroup variant was built in r02, lost 140 vs 58 ms on the heavy rounds, and was removed in r03); its light targets
    // alone go through one workgroup each first (dh_fz_light_kernel, dh_light_prepass).
    static const bool mi_rounds = fw_mi_rounds();
    // (more than 65 535 samples: 32-bit cell counts -- r04: the persistent kernel has a 32-bit-count form too, PRE = 2)
    y.nzk = c->P.kind == FW_FZ_NZ;
    y.fz = fz_kind;
    y.per_target = !fz_kind && !mi_rounds;
    // interleaving-phase look-ahead (first windows of the next candidates, same accepted list): FW_DH_SPEC0 candidates,
    // only while the last launch held fewer than FW_DH_SPEC0_BELOW ranks and fewer than FW_DH_SPEC0_JOBS jobs -- it
    // pays where the rounds are latency-bound, i.e. on a rank of a multi-GPU job (one rank of 8: 103.6 -> 95.2 ms,
    // one of 2: 208 -> 204.7 ms) and in the tail of a single-GPU pass (315.8 -> 314.2 ms)
    static const int spec0_env = fw_knob_int(knob::FW_DH_SPEC0, 2);
    y.spec0_depth = c->P.kind == FW_FZ ? std::min(std::max(spec0_env, 0), DH_MAX_SPEC) : 0;
    // segments per launch by launch size (fz): below FW_SEG_A ranks a third of seg_target, below FW_SEG_B two thirds.
    // cfg3, ms per pass on one GPU / one rank of 2 / of 8: fixed 3 072: 298.8 / 200.3 / 94.9; A, B = 4M, 8M: 295.8 /
    // 194.4 / 82.3; 6M, 10M: 295.8 / 192.8 / 80.3; 8M, 12M: 295.1 / 193.7 / 79.8 (fixed 1 024: 81.1 for the rank of 8
    // but 221 for the rank of 2; 512: 102)
    static const unsigned long long seg_a_env = fw_knob_u64(knob::FW_SEG_A, 8000000ull);
    static const unsigned long long seg_b_env = fw_knob_u64(knob::FW_SEG_B, 12000000ull);
    y.seg_a = fz_kind ? seg_a_env : 0ull;
    y.seg_b = fz_kind ? seg_b_env : 0ull;
    // striding workgroups of the segment kernel.  FW_SEG_GRID caps them (experiment: with fewer workgroups than resident
    // slots the one-workgroup step / plan kernels of the OTHER chain find a free CU at once instead of queueing behind
    // this launch's pending workgroups -- cfg5 profile: dh_plan_kernel 6.3 ms per call, all of it waiting)
    static const unsigned seg_grid_env = (unsigned)fw_knob_pos(knob::FW_SEG_GRID, 0ull);
    // r06 (cfg3, one box): 3 584 workgroups 152.6 ms / ff = 0 135.2; 2 560: 151.6 / 133.3; 2 304: 150.6 / 132.2; **2 048: 149.3 / 131.8**; 1 792: 151.7 / 135.6; 1 536: 157.6; 1 024: 164 -- two
    // resident sets of the size-3 table kernel (256 CUs x 4 workgroups), the rest of the list by striding (profiles/r06_cfg3_segment_grid.txt).  max_k > 3 and fz_nz: not measured, as before.
    const unsigned grid_dflt = (c->P.kind == FW_FZ && c->P.max_k <= 3) ? std::min(y.seg_target + 512u, 2048u) : y.seg_target + 512u;
    y.grid_seg = seg_grid_env ? std::min(y.seg_target + 512u, seg_grid_env) : grid_dflt;
    // FW_DH_LOG=<file>: one line per planned launch (ranks, live jobs, segments) -- profiling aid, see profiles/README.md
    static const char *log_path = fw_knob_str(knob::FW_DH_LOG);
    y.log_path = log_path;
    // Rounds per batch.  The host sees "every target has finished" one batch late, so a pass of few, light targets (a rank of an
    // 8-rank job holds 128 targets per feed-forward round at cfg3, 15 dependent rounds) ran 33 rounds, half of them empty: short
    // batches for short lists (r03: 1.05 -> 0.75 ms per light round; the host enqueues 4 rounds in ~60 us, a round takes 25-100 us)
    static const int nb_env = std::min((int)fw_knob_pos(knob::FW_DH_BATCH, 0ull), DH_BATCH);
    y.nb = nb_env ? nb_env : (ntg <= 1024 ? 4 : DH_BATCH);
    // Kernel timing (fw_counters.t_dev_subsets_s): HIP events around one segment launch in FW_DH_TIME_EVERY (default 4),
    // the sampled slot rotating from batch to batch so that every position of the 16-round batch is covered; the
    // sampled average is scaled to all non-empty launches.  Every event pair costs ~12 us of idle GPU around the launch
    // (rocprofv3 trace: 5.9 us before + 5.7 us after, back-to-back otherwise): cfg3, ms per pass / average launch us at
    // k = 1: 275.3 / 224.2, k = 2: 272.2 / 224.5, k = 4: 270.4 / 224.5, k = 8: 270.2 / 224.8 -- same average, 2 % less time.
    static const int time_every = (int)fw_knob_pos(knob::FW_DH_TIME_EVERY, 4ull);
    y.time_every = time_every;
    // FW_DH_HP=1: the small kernels of a round on the chain's high-priority stream (fw_ctx::dh_hp_stream) -- an experiment kept behind its knob
    static const int hp_env = fw_knob_int(knob::FW_DH_HP, -1);
    y.use_hp = !y.per_target && hp_env > 0;  // (measured at cfg5: no effect -- what held the plan kernel back was its size, not its queue; default off)
    static const bool plan_small = fw_knob_on(knob::FW_DH_PLAN_SMALL);  // (0: the 1 024-thread dh_plan_kernel)
    y.plan_small = plan_small;
    return y;
}

static unsigned dh_team_min() { static const unsigned v = (unsigned)fw_knob_int(knob::FW_MI_TEAM_MIN, 96); return v; }
static unsigned dh_team_max() { static const unsigned v = (unsigned)fw_knob_int(knob::FW_MI_TEAM_MAX, 192); return v; }  // (64 / 256: cfg2 10.5 ms, cfg4 161.7; 128 / 128: 9.4, 162.7; 96 / 192: 9.3, 159.6)
// order of a discrete round's n targets: heaviest first, stable (deg(t) = candidates of target t).  Returns the team size: the first
// targets of the order with at least FW_MI_TEAM_MIN candidates, at most FW_MI_TEAM_MAX of them, get a workgroup each
template <class Deg>
static unsigned dh_heaviest_first(int32_t *order, int n, Deg deg)
{
    for (int t = 0; t < n; ++t) order[t] = t;
    std::stable_sort(order, order + n, [&](int32_t u, int32_t v) { return deg(u) > deg(v); });
    const unsigned team_min = dh_team_min(), team_max = dh_team_max();
    unsigned team = 0u;
    while (team_min > 0u && team < team_max && (int)team < n && (unsigned)deg(order[team]) >= team_min) ++team;
    return team;
}

// launches the persistent discrete kernel over targets tg[0 .. ntg) taken in the order d_order (heaviest first; the first `team` of
// them by a workgroup each); returns the grid.  The queue and the boards must be zero (the caller's memsets on the same stream).
static unsigned dh_mi_launch(fw_ctx *c, hipStream_t st, DhTgt *d_tg, int ntg, const int32_t *d_order, const DhArrays &A, DhParams P, unsigned team,
                             bool trace_host, MiQueue *d_mq, MiBoard *d_boards, FwSegOut *d_mres, int32_t *d_bacc)
{
    MiDev M = fwi_mi_dev(c);
    M.view = M.dense && M.nzmode && c->mi_view;  // HITON-PC under the dense rules tests on row views (hiton.jl:41-50)
    // as many workgroups as stay resident (one per CU: the test routine needs ~260 VGPRs, one wavefront per SIMD; cfg4:
    // 62 ms with one, 71 ms with two requested): the wavefronts fetch targets themselves
    static const unsigned wg_per_cu = (unsigned)fw_knob_pos(knob::FW_MI_WG_PER_CU, 1ull);
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->P.device);
    const unsigned grid = std::min((unsigned)((ntg + 3) / 4), wg_per_cu * (unsigned)n_cu);
    static const unsigned team_steps = (unsigned)fw_knob_int(knob::FW_MI_TEAM_STEPS, 2);
    static const unsigned team_tail = (unsigned)fw_knob_int(knob::FW_MI_TEAM_TAIL, 0);
    P.mi_team = team;
    P.mi_team_steps = team_steps;
    P.mi_team_tail = team_tail;
#ifdef FW_MI_TICKS
    P.mi_trace = 1u;
#else
    P.mi_trace = trace_host ? 1u : 0u;
#endif
#define DH_MI_LAUNCH(LL, NN, PP, RR)                                                                                                  \
    do {                                                                                                                              \
        if (A.rej)                                                                                                                    \
            hipLaunchKernelGGL((dh_mi_target_kernel<LL, NN, PP, RR, false, true>), dim3(grid), dim3(256), 0, st, d_tg, ntg, d_order, \
                               A, M, P, d_mq, d_boards, d_mres, d_bacc);                                                              \
        else if (P.elim_mode != 0)                                                                                                    \
            hipLaunchKernelGGL((dh_mi_target_kernel<LL, NN, PP, RR, true, false>), dim3(grid), dim3(256), 0, st, d_tg, ntg, d_order, \
                               A, M, P, d_mq, d_boards, d_mres, d_bacc);                                                              \
        else                                                                                                                          \
            hipLaunchKernelGGL((dh_mi_target_kernel<LL, NN, PP, RR, false, false>), dim3(grid), dim3(256), 0, st, d_tg, ntg, d_order,\
                               A, M, P, d_mq, d_boards, d_mres, d_bacc);                                                              \
    } while (0)
    const bool pre = c->P.n <= MI_PRE_N && c->P.max_k <= MI_PRE_K;
    // four subsets per wavefront step (mi_test_core4): n <= 5120, max_k <= 3, 2 x 2 cells per stratum.  FW_MI_ROW4=0: one per step
    static const bool row4_env = fw_knob_on(knob::FW_MI_ROW4);
    // ... used up to 2048 samples (four words per lane): cfg2 (n = 500) 15.2 -> 12.5 ms.  At cfg4's n = 5000 a step of four
    // tests takes as long as four one-test steps (34 us: ten words per lane, 390 registers with the spills parked in AGPRs),
    // and since most jobs stop at their first test the three speculative ones are pure cost: measured 56.2 vs 56.8 ms on one
    // GPU, 35.3 vs 39.2 ms for one rank of eight -- FW_MI_ROW4=2 forces it on up to MI4_N for such experiments
    static const bool row4_force = fw_knob_int(knob::FW_MI_ROW4, 1) == 2;
    const bool r4 = row4_env && pre && c->P.n <= (row4_force ? MI4_N : 2048) && (c->L == 2 || c->mi_nxy == 2);
    const bool wide = c->P.n > 65535;  // cell counts beyond 16 bits: one count per register, 32-bit tables (mi_test_core<.., WIDE>)
    if (c->L == 2) {
        if (wide) DH_MI_LAUNCH(2, 2, 2, false); else if (r4) DH_MI_LAUNCH(2, 2, 1, true); else if (pre) DH_MI_LAUNCH(2, 2, 1, false); else DH_MI_LAUNCH(2, 2, 0, false);
    } else if (c->mi_nxy == 2) {
        if (wide) DH_MI_LAUNCH(3, 2, 2, false); else if (r4) DH_MI_LAUNCH(3, 2, 1, true); else if (pre) DH_MI_LAUNCH(3, 2, 1, false); else DH_MI_LAUNCH(3, 2, 0, false);
    } else {
        if (wide) DH_MI_LAUNCH(3, 3, 2, false); else if (pre) DH_MI_LAUNCH(3, 3, 1, false); else DH_MI_LAUNCH(3, 3, 0, false);
    }
#undef DH_MI_LAUNCH
    return grid;
}

static void dh_mi_trace(const MiQueue &hq, unsigned grid)
{
    const double nw = 4.0 * (double)grid, ms = 1e-5;
    if (hq.tick[1])
        fprintf(stderr, "[fw] test routine: %llu calls, %llu tests (mean set size %.2f); per test %.2f us before the core (unranking, list), %.2f us in the core, %.2f us in the accounting (Q)\n",
                hq.tick[0], hq.tick[1], (double)hq.tick[5] / (double)hq.tick[1], 1e-2 * hq.tick[2] / (double)hq.tick[1],
                1e-2 * hq.tick[3] / (double)hq.tick[1], 1e-2 * hq.tick[4] / (double)hq.tick[1]);
    if (hq.tick[1])
        fprintf(stderr, "[fw] state machine, ms per wavefront: dh_advance %.3f, job set-up %.3f, commit + counters %.3f, publish %.3f, idle wait for own board %.3f, merge %.3f; "
                        "test routine: before the core %.3f, core %.3f, accounting %.3f\n",
                ms * hq.tick[6] / nw, ms * hq.tick[7] / nw, ms * hq.tick[8] / nw, ms * hq.tick[9] / nw, ms * hq.tick[10] / nw, ms * hq.tick[11] / nw,
                ms * hq.tick[2] / nw, ms * hq.tick[3] / nw, ms * hq.tick[4] / nw);
    if (hq.tm_steps)
        fprintf(stderr, "[fw] team rounds: %llu wavefront-rounds, %llu tests in them; per wavefront-round %.2f us in the test routine, %.2f us at the barrier\n",
                hq.tm_steps, hq.tm_tests, 1e-2 * hq.tm_run / (double)hq.tm_steps, 1e-2 * hq.tm_wait / (double)hq.tm_steps);
    fprintf(stderr, "[fw] boards %u records %u; per wavefront (%u wavefronts): until out of targets %.2f ms = own first tests %.2f + board phases %.2f + helping before jobs %.2f + state machine %.2f; tail %.2f ms\n",
            hq.n_boards, hq.res_top, 4u * grid, ms * hq.t_total / nw, ms * hq.t_body / nw, ms * hq.t_ctl / nw, ms * hq.t_sleep / nw,
            ms * ((double)hq.t_total - (double)hq.t_body - (double)hq.t_ctl - (double)hq.t_sleep) / nw, ms * hq.n_seg / nw);
}

// watchdog word of a finished persistent launch -> error; else its trace under FW_TRACE_HOST
static int dh_mi_check(fw_ctx *c, const MiQueue &hq, unsigned grid, int round, int ntg, bool trace_host)
{
    if (hq.pad[0])
        return fw_fail(c, FW_ERR_DEVICE, "discrete HITON kernel, round %d: watchdog %u (boards %u, targets done %u of %d)", round, hq.pad[0], hq.n_boards, hq.targets_done, ntg);
    if (trace_host) dh_mi_trace(hq, grid);
    return FW_OK;
}

// ---- device buffers that the drivers share ----

// a target's persistent lists (TPC / PC with statistics and p-values, accepted lists, whitelist), n entries in all; the accepted lists
// take 2 * n entries in each of acc_d1 buffers (DH_ACC_OFF)
struct DhLists {
    int32_t *tpc_key, *pc_key, *acc, *wl;
    double *tpc_stat, *tpc_p, *pc_stat, *pc_p;
};
static DhLists dh_lists_layout(DhArena &a, size_t n, size_t acc_d1, size_t n_wl)
{
    DhLists b{};
    b.tpc_key = a.take<int32_t>(n, 4);
    b.pc_key = a.take<int32_t>(n, 4);
    b.acc = a.take<int32_t>(2 * n * acc_d1, 4);
    b.tpc_stat = a.take<double>(n, 8);
    b.tpc_p = a.take<double>(n, 8);
    b.pc_stat = a.take<double>(n, 8);
    b.pc_p = a.take<double>(n, 8);
    b.wl = a.take<int32_t>(n_wl, 4);
    return b;
}

// what the rounds of the segment kernel over ntg targets work in (DhRounds): a round of fwi_devhiton_run has its own, a chain of
// fwi_devhiton_fz_schedule reserves one for its largest round
struct DhRoundScratch {
    DhGlobal *g;
    long long *seg0;
    unsigned long long *win, *win2;
    unsigned int *sp;
    int32_t *act;  // ping-pong list of the unfinished targets
    FwSeg *segs;
    FwSegOut *so;
    float *tmat;
};
static DhRoundScratch dh_scratch_layout(DhArena &a, size_t ntg, size_t max_ns, size_t tm_floats)
{
    DhRoundScratch b{};
    b.g = a.take<DhGlobal>(1);
    b.seg0 = a.take<long long>(ntg + 1);
    b.win = a.take<unsigned long long>(ntg + 1);
    b.sp = a.take<unsigned int>(ntg + 1);
    b.win2 = a.take<unsigned long long>(ntg + 1);
    b.act = a.take<int32_t>(2 * ntg);
    b.segs = a.take<FwSeg>(max_ns);
    b.so = a.take<FwSegOut>(max_ns);
    if (tm_floats) b.tmat = a.take<float>(tm_floats, 4);
    return b;
}

// a copy of the level-0 lists
struct DhLevel0 {
    long long *off;
    int32_t *idx;
    double *stat, *p;
};

// The arrays the kernels work on: the interleaving candidates, a driver's state and the level-0 lists -- the context's where it holds
// them on the device, else the run's own copy.  wl_cnt and tmat stay null: the drivers that have them set them.
static DhArrays dh_arrays(const fw_ctx *c, const int32_t *cand0, const DhLists &s, const DhLevel0 &own)
{
    const bool nb_on_dev = c->d_nb_idx != nullptr;
    DhArrays A{};
    A.cand0 = cand0;
    A.tpc_key = s.tpc_key;
    A.pc_key = s.pc_key;
    A.acc = s.acc;
    A.tpc_stat = s.tpc_stat;
    A.tpc_p = s.tpc_p;
    A.pc_stat = s.pc_stat;
    A.pc_p = s.pc_p;
    A.wl = s.wl;
    A.nb_off = nb_on_dev ? c->d_nb_off : own.off;
    A.nb_idx = nb_on_dev ? c->d_nb_idx : own.idx;
    A.nb_stat = nb_on_dev ? c->d_nb_stat : own.stat;
    A.nb_p = nb_on_dev ? c->d_nb_p : own.p;
    A.rej = c->d_rej_run;
    return A;
}

// ---- one round of targets (fwi_devhiton_run) ----

// what sizes the arena of a round
struct DhRunSizes {
    size_t ntg, tot, d1, n_wl, max_ns, tm_floats, nz_arena, p, nnz;
    bool log, per_target, nzk, own_nb;
};
struct DhRunBufs {
    DhTgt *tg;
    DhRoundScratch s;
    int32_t *cand0;
    DhLists lists;
    ulonglong2 *log;
    MiQueue *mq;  // persistent kernel only
    MiBoard *boards;
    FwSegOut *mres;
    int32_t *bacc;
    FwNzJob *nzrecs;  // fz_nz only
    long long *nzaoff;
    float *nzarena;
    DhLevel0 nb;  // own copy of the level-0 lists: only when the context holds none on the device
};
static DhRunBufs dh_run_layout(DhArena &a, const DhRunSizes &z)
{
    DhRunBufs b{};
    b.tg = a.take<DhTgt>(z.ntg);
    b.s = dh_scratch_layout(a, z.ntg, z.max_ns, z.tm_floats);
    b.cand0 = a.take<int32_t>(z.tot, 4);
    b.lists = dh_lists_layout(a, z.tot, z.d1, z.n_wl);
    if (z.log) b.log = a.take<ulonglong2>(DH_LOG_CAP);
    if (z.per_target) {
        b.mq = a.take<MiQueue>(1);
        b.boards = a.take<MiBoard>(MI_BOARD_CAP);
        b.mres = a.take<FwSegOut>(MI_REC_CAP);
        b.bacc = a.take<int32_t>(MI_BACC_CAP);
    }
    if (z.nzk) {
        b.nzrecs = a.take<FwNzJob>(z.ntg);
        b.nzaoff = a.take<long long>(z.ntg);
        b.nzarena = a.take<float>(z.nz_arena, 4);
    }
    if (z.own_nb) {
        b.nb.off = a.take<long long>(z.p + 1);
        b.nb.idx = a.take<int32_t>(z.nnz, 4);
        b.nb.stat = a.take<double>(z.nnz, 8);
        b.nb.p = a.take<double>(z.nnz, 8);
    }
    return b;
}

struct DhRun {
    fw_ctx *c;
    int chain, ntg;
    hipStream_t st;
    bool trace_host;
    DhPolicy y;
    // host-side layout (dh_build_targets)
    bool use_devc;  // candidate lists built on the device (fw_bh.hip)
    std::vector<DhTgt> tg;
    std::vector<int32_t> cand0, wl;
    std::vector<long long> nz_aoff;
    size_t tot = 0, tm_floats = 0, nz_arena = 0;
    int max_cap = 0, max_wl = 0;  // most candidates / most whitelisted neighbours of one target
    unsigned max_ns = 0;          // capacity of the segment list (dh_max_ns)
    // device side (dh_upload)
    DhRunBufs D{};
    DhGlobal *hg = nullptr;  // two pinned copies of the device record (one per batch in flight)
    DhArrays A{};
    DhParams P{};
    // what the launches report
    double timed_s = 0.0;
    long timed_n = 0, launches_n = 0;
    long light_n = 0;  // launches of dh_fz_light_kernel (dh_light_prepass): a launch of the segment body that is one kernel, not four
    std::vector<float> log_ms;  // FW_DH_LOG: segment-kernel time of launch i (planned by plan #i)
    unsigned max_a_seen = 0;    // longest accepted list reported so far (lags by up to two batches)
    unsigned max_ab_seen = 0;   // ... and the largest accepted + whitelisted-to-come
    bool dev_wl = false;        // fwi_devhiton_fz_schedule: the whitelists were built on the device (R.wl stays empty), the longest holds max_wl entries
};

// The layout rule of a round of targets, for the host-built rounds (dh_build_targets) and the slots of fwi_devhiton_fz_schedule alike.
// dh_tm_off: the offset (floats) of the local correlation matrix of a target with deg level-0 neighbours in its round's block, which
// holds tm_floats so far and grows by the matrix; -1: the target gets none (dh_tmat_build_kernel fills the others)
static long long dh_tm_off(const fw_ctx *c, const DhPolicy &y, int deg, size_t &tm_floats)
{
    const bool tm_on = c->P.kind == FW_FZ && c->P.max_k <= 5 && c->d_cor != nullptr && y.tm_min > 0;  // (max_k 6-7: the general-form kernel reads the p x p matrix)
    const size_t m = (size_t)deg + 1;
    if (!tm_on || deg < y.tm_min || m > 4096 || tm_floats + m * m > (size_t)1 << 32) return -1;  // (<= 16 GB per chain; ids of a target staged in 16 KB of LDS)
    const long long off = (long long)tm_floats;
    tm_floats += m * m;
    return off;
}
// capacity of the segment list of a round of ntg targets (a job + its look-ahead jobs each round up)
static unsigned dh_max_ns(const DhPolicy &y, int ntg) { return y.seg_target + (unsigned)ntg * (unsigned)(1 + DH_MAX_SPEC) + 256u; }

// targets, candidate lists and whitelists in one flat layout each; offsets of the local matrices
static void dh_build_targets(DhRun &R, const std::vector<FwDhTarget> &in)
{
    const fw_ctx *c = R.c;
    const int ntg = R.ntg;
    R.use_devc = in[0].nc_dev >= 0 && c->d_cand != nullptr;
    R.tg.resize((size_t)ntg);
    long long co = 0, wo = 0;
    for (int t = 0; t < ntg; ++t) {
        DhTgt x{};
        x.T = in[t].T;
        x.nc = R.use_devc ? in[t].nc_dev : (int32_t)in[t].cands.size();
        x.cap = x.nc;
        x.cand_off = R.use_devc ? c->nb_off[in[t].T] : co;
        x.phase = x.nc == 0 ? 2 : 0;
        x.co = co;
        x.wl_off = wo;
        x.wl_n = in[t].wl_n;
        x.nb_off = c->nb_off[x.T];
        x.nb_n = (int32_t)(c->nb_off[x.T + 1] - c->nb_off[x.T]);
        if (!R.use_devc) R.cand0.insert(R.cand0.end(), in[t].cands.begin(), in[t].cands.end());
        if (in[t].wl_n) R.wl.insert(R.wl.end(), in[t].wl, in[t].wl + in[t].wl_n);
        co += x.nc;
        wo += in[t].wl_n;
        R.max_cap = std::max(R.max_cap, x.nc);
        R.max_wl = std::max(R.max_wl, (int)in[t].wl_n);
        R.tg[t] = x;
    }
    R.tot = (size_t)co;
    for (int t = 0; t < ntg; ++t) R.tg[t].tm_off = dh_tm_off(c, R.y, R.tg[t].nb_n, R.tm_floats);
    // fz_nz: a record and an arena slice of (longest list + 2)^2 floats per target.  Without whitelists an accepted list never outgrows
    // the candidate list; with whitelists (feed-forward) a whitelisted member of the elimination pool is pushed a second time
    // (hiton.jl:24-26), so a list can reach twice the candidates -- the capacity of the accepted buffers (DH_ACC_OFF: 2 x cap)
    if (R.y.nzk) {
        R.nz_aoff.resize((size_t)ntg);
        for (int t = 0; t < ntg; ++t) {
            R.nz_aoff[t] = (long long)R.nz_arena;
            const size_t mt = (size_t)(R.wl.empty() ? 1 : 2) * (size_t)R.tg[t].nc + 2;
            R.nz_arena += mt * mt;
        }
    }
    R.max_ns = dh_max_ns(R.y, ntg);
}

// device buffers (one arena), the round's inputs, the local correlation matrices, the run's parameters
static int dh_upload(DhRun &R)
{
    fw_ctx *c = R.c;
    hipStream_t st = R.st;
    const int ntg = R.ntg, p = c->P.p;
    const size_t tot = R.tot, nnz = (size_t)c->nb_off[p];
    const bool nb_on_dev = c->d_nb_idx != nullptr;  // (else the run carries its own copy: dh_arrays)
    const DhRunSizes z{(size_t)ntg, tot, (size_t)R.y.spec_depth + 1, R.wl.size(), R.max_ns, R.tm_floats, R.nz_arena, (size_t)p, nnz,
                       R.y.log_path != nullptr, R.y.per_target, R.y.nzk, !nb_on_dev};
    int rc;
    if ((rc = dh_arena_reserve(c, c->d_dh[R.chain], dh_run_layout, z, &R.D))) return rc;
    if ((rc = fw_pin_reserve(c, c->h_dh[R.chain], 4096))) return rc;
    const DhRunBufs &D = R.D;
    DhGlobal *hg = R.hg = (DhGlobal *)c->h_dh[R.chain].ptr;
    memset(hg, 0, 2 * sizeof(DhGlobal));
    if (R.y.nzk) {
        FW_HIP(c, hipMemcpyAsync(D.nzaoff, R.nz_aoff.data(), sizeof(long long) * (size_t)ntg, hipMemcpyHostToDevice, st));
        FW_HIP(c, hipMemsetAsync(D.nzrecs, 0xff, sizeof(FwNzJob) * (size_t)ntg, st));  // (pad bit 0 set: nothing to compute until a job writes its record)
    }
    FW_HIP(c, hipMemcpyAsync(D.tg, R.tg.data(), sizeof(DhTgt) * ntg, hipMemcpyHostToDevice, st));
    hg[0].n_act = (unsigned int)ntg;  // every target starts on the list (the pinned page is the staging copy: stream-ordered)
    FW_HIP(c, hipMemcpyAsync(D.s.g, hg, sizeof(DhGlobal), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dh_iota_kernel, dim3((unsigned)((ntg + 255) / 256)), dim3(256), 0, st, D.s.act, ntg);  // (was a blocking copy of a host list)
    FW_HIP(c, hipMemsetAsync(D.s.seg0, 0, sizeof(long long) * ((size_t)ntg + 1), st));
    if (tot && !R.use_devc) FW_HIP(c, hipMemcpyAsync(D.cand0, R.cand0.data(), 4 * tot, hipMemcpyHostToDevice, st));
    if (!R.wl.empty()) FW_HIP(c, hipMemcpyAsync(D.lists.wl, R.wl.data(), 4 * R.wl.size(), hipMemcpyHostToDevice, st));
    if (!nb_on_dev) {
        FW_HIP(c, hipMemcpyAsync(D.nb.off, c->nb_off.data(), 8 * ((size_t)p + 1), hipMemcpyHostToDevice, st));
        if (nnz) {
            FW_HIP(c, hipMemcpyAsync(D.nb.idx, c->nb_idx.data(), 4 * nnz, hipMemcpyHostToDevice, st));
            FW_HIP(c, hipMemcpyAsync(D.nb.stat, c->nb_stat.data(), 8 * nnz, hipMemcpyHostToDevice, st));
            FW_HIP(c, hipMemcpyAsync(D.nb.p, c->nb_p.data(), 8 * nnz, hipMemcpyHostToDevice, st));
        }
    }
    DhArrays &A = R.A = dh_arrays(c, R.use_devc ? c->d_cand : D.cand0, D.lists, D.nb);
    A.tmat = D.s.tmat;
    if (D.s.tmat) {
        hipLaunchKernelGGL(dh_tmat_build_kernel, dim3((unsigned)ntg, 8u), dim3(256), 0, st, (const DhTgt *)D.tg, ntg, A.nb_idx, (const float *)c->d_cor, p, D.s.tmat);
        FW_HIP(c, hipGetLastError());
        if (R.trace_host) fprintf(stderr, "[fw] chain %d: local correlation matrices: %.1f MB\n", R.chain, 4e-6 * (double)R.tm_floats);
    }
    R.P = dh_make_params(c, ntg, R.y.spec_depth, R.y.spec0_depth);
    return FW_OK;
}

// discrete kinds: the whole round as one persistent launch (dh_mi_target_kernel)
static int dh_run_persistent(DhRun &R, DhEvents &E)
{
    fw_ctx *c = R.c;
    hipStream_t st = R.st;
    const int ntg = R.ntg;
    const DhRunBufs &D = R.D;
    const std::vector<DhTgt> &tg = R.tg;
    std::vector<int32_t> order((size_t)ntg);
    const unsigned team = dh_heaviest_first(order.data(), ntg, [&](int32_t t) { return tg[t].nc; });
    FW_HIP(c, hipMemcpyAsync(D.s.act, order.data(), sizeof(int32_t) * (size_t)ntg, hipMemcpyHostToDevice, st));
    if (R.trace_host) {
        int c32 = 0, c64 = 0, c128 = 0, c192 = 0;
        for (int t = 0; t < ntg; ++t) c32 += tg[t].nc >= 32, c64 += tg[t].nc >= 64, c128 += tg[t].nc >= 128, c192 += tg[t].nc >= 192;
        fprintf(stderr, "[fw] chain %d: %u targets run by a workgroup each (>= %u candidates); targets with >= 32 / 64 / 128 / 192 candidates: %d / %d / %d / %d; "
                        "candidates of the 1st / 64th / 256th heaviest: %d / %d / %d\n", R.chain, team, dh_team_min(), c32, c64, c128, c192,
                tg[order[0]].nc, ntg > 63 ? tg[order[63]].nc : -1, ntg > 255 ? tg[order[255]].nc : -1);
    }
    FW_HIP(c, hipMemsetAsync(D.mq, 0, sizeof(MiQueue), st));
    FW_HIP(c, hipMemsetAsync(D.boards, 0, sizeof(MiBoard) * MI_BOARD_CAP, st));  // ready flags, claimed / finished counts
    FW_HIP(c, hipEventRecord(E.ev[0], st));
    const unsigned grid = dh_mi_launch(c, st, D.tg, ntg, (const int32_t *)D.s.act, R.A, R.P, team, R.trace_host, D.mq, D.boards, D.mres, D.bacc);
    FW_HIP(c, hipGetLastError());
    FW_HIP(c, hipEventRecord(E.ev[1], st));
    FW_HIP(c, hipStreamSynchronize(st));
    MiQueue hq{};
    FW_HIP(c, hipMemcpy(&hq, D.mq, sizeof(hq), hipMemcpyDeviceToHost));
    if (int rc = dh_mi_check(c, hq, grid, 0, ntg, R.trace_host)) return rc;
    float ms = 0.0f;
    FW_HIP(c, hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
    R.timed_s = 1e-3 * (double)ms;
    R.timed_n = R.launches_n = 1;
    return FW_OK;
}

// Fisher-z kinds (and the discrete ones under FW_MI_ROUNDS): rounds of segment kernel -> step -> (compact) -> plan -> fill, enqueued in
// batches.  Two batches are kept in flight: the host enqueues batch b + 1 before it waits for the end of batch b, so the GPU
// never runs dry while the host looks at the round record (a stream synchronisation per batch left ~200 us of
// idle GPU per 16 rounds).  Rounds after the last one are no-ops (no live segment, nothing to merge).
struct DhRounds {
    DhRun &R;
    DhEvents &E;  // E.ev[(q * DH_BATCH + r) * 2 + 0 / 1] around the segment launch of round r of batch slot q; E.ev_end[q]
    fw_ctx *c = R.c;
    const DhRunBufs &D = R.D;
    const DhRoundScratch &S = R.D.s;
    const DhPolicy &y = R.y;
    const int ntg = R.ntg;
    hipStream_t st = R.st, hs = R.st;  // hs: stream of the small kernels (FW_DH_HP: the chain's high-priority stream)
    DhPlanArgs PA{};
    // The in-lane kernel (accepted lists beyond FW_TAB_A) is only launched when such a list can exist in the coming batch:
    // without whitelists an accepted list grows by at most one entry per round, so max_a (longest list so far, read
    // back once per batch) + BATCH bounds it; with whitelists a round can append several entries -> static bound.
    const bool any_wl = !R.wl.empty() || (R.dev_wl && R.max_wl > 0);
    const bool any_big_static = (any_wl ? 2 * R.max_cap : R.max_cap) > FW_TAB_A;
    const unsigned g_fill = (R.max_ns + 255) / 256;
    unsigned n_act_bound = (unsigned)R.ntg;  // unfinished targets as of the last record read (only ever shrinks)
    bool big_skipped[2] = {false, false};    // per batch slot: some round of it ran without the in-lane kernel

    DhRounds(DhRun &r, DhEvents &e) : R(r), E(e)
    {
        PA.seg_target = y.seg_target;
        PA.seg_q = R.P.seg_q;
        PA.seg_min = R.P.seg_min;
        PA.log_cap = DH_LOG_CAP;
        PA.log = D.log;
        PA.seg_a = y.seg_a;
        PA.seg_b = y.seg_b;
    }
    hipEvent_t &ev(int q, int i) { return E.ev[(size_t)(q * 2 * DH_BATCH + i)]; }
    bool timed(unsigned b, int r) const { return ((r + (int)(b % (unsigned)y.time_every)) % y.time_every) == 0; }  // the sampled slot rotates from batch to batch

    int hp_stream()
    {
        const int chain = R.chain;
        if (!c->dh_hp_stream[chain]) {
            int lo = 0, hi = 0;
            FW_HIP(c, hipDeviceGetStreamPriorityRange(&lo, &hi));  // (hi: numerically lowest = highest priority)
            FW_HIP(c, hipStreamCreateWithPriority(&c->dh_hp_stream[chain], hipStreamNonBlocking, hi));
            for (int e = 0; e < 2; ++e) FW_HIP(c, hipEventCreateWithFlags(&c->dh_hp_ev[chain][e], hipEventDisableTiming));
        }
        hs = c->dh_hp_stream[chain];
        return FW_OK;
    }
    // the small kernels between two segment launches: merge + advance, (compact,) plan, fill
    int planfill(bool compact)
    {
        const DhArrays &A = R.A;
        if (y.use_hp) {  // behind the segment kernel of this round ...
            FW_HIP(c, hipEventRecord(c->dh_hp_ev[R.chain][0], st));
            FW_HIP(c, hipStreamWaitEvent(hs, c->dh_hp_ev[R.chain][0], 0));
        }
        if (A.rej)  // (the rejection log: its own instantiation, so that the default one keeps its registers)
            hipLaunchKernelGGL(dh_step_kernel<true>, dim3((n_act_bound + 3u) / 4u), dim3(256), 0, hs, D.tg, ntg, S.g, A,
                               (const FwSegOut *)S.so, (const long long *)S.seg0, S.win, S.sp, S.win2, (const int32_t *)S.act, R.P);
        else
            hipLaunchKernelGGL(dh_step_kernel<false>, dim3((n_act_bound + 3u) / 4u), dim3(256), 0, hs, D.tg, ntg, S.g, A,
                               (const FwSegOut *)S.so, (const long long *)S.seg0, S.win, S.sp, S.win2, (const int32_t *)S.act, R.P);
        if (compact)  // between step and plan: seg0 of the coming launch is built on the new list
            hipLaunchKernelGGL(dh_compact_kernel, dim3(1), dim3(1024), 0, hs, (const DhTgt *)D.tg, ntg, S.g, S.act);
        if (y.plan_small)
            hipLaunchKernelGGL(dh_plan_small_kernel, dim3(1), dim3(256), 0, hs, ntg, S.g, (const unsigned long long *)S.win,
                               (const unsigned int *)S.sp, (const unsigned long long *)S.win2, (const int32_t *)S.act, S.seg0, PA);
        else
            hipLaunchKernelGGL(dh_plan_kernel, dim3(1), dim3(1024), 0, hs, ntg, S.g, (const unsigned long long *)S.win,
                               (const unsigned int *)S.sp, (const unsigned long long *)S.win2, (const int32_t *)S.act, S.seg0, PA);
        hipLaunchKernelGGL(dh_fill_kernel, dim3(g_fill), dim3(256), 0, hs, (const DhTgt *)D.tg, ntg, S.g,
                           (const long long *)S.seg0, A, S.segs, y.spec_depth + 1, (const int32_t *)S.act);
        if (y.use_hp) {  // ... and in front of the next one
            FW_HIP(c, hipEventRecord(c->dh_hp_ev[R.chain][1], hs));
            FW_HIP(c, hipStreamWaitEvent(st, c->dh_hp_ev[R.chain][1], 0));
        }
        return FW_OK;
    }
    int enqueue_batch(unsigned b)
    {
        const DhArrays &A = R.A;
        const int q = (int)(b & 1u);
        const unsigned *d_ns = &S.g->ns;
        for (int r = 0; r < y.nb; ++r) {
            // lists grow by at most one entry per round: 3 batches cover the lag of the record plus this batch
            // ... and a whitelisted neighbour is appended at most once per target: max_ab (accepted + whitelisted neighbours
            // still to come, maximum over the targets, kept by dh_step_kernel) bounds what whitelists can add.  (r02
            // profile: with whitelists the in-lane kernel was launched every round "in case" and left on the device flag --
            // 16 us of every round's critical path, 26 ms per chain and pass at cfg3.)
            const bool any_big = any_big_static && R.max_ab_seen + 3u * (unsigned)DH_BATCH + 1u > (unsigned)FW_TAB_A;
            if (r == 0) big_skipped[q] = false;
            if (!any_big) big_skipped[q] = true;
            if (timed(b, r)) (void)hipEventRecord(ev(q, 2 * r), st);
            // discrete segment kernel: one workgroup per record, no stride loop -> the grid follows the bound on the list
            const unsigned grid_mi = std::min(R.max_ns, y.seg_target + n_act_bound * (unsigned)(1 + std::max(y.spec_depth, y.spec0_depth)) + 256u);
            int rc;
            if (y.nzk) {
                // this round's fresh jobs: records (one thread per unfinished target), their matrices, then the enumeration
                hipLaunchKernelGGL(dh_nz_recs_kernel, dim3((n_act_bound + 255u) / 256u), dim3(256), 0, st, (const DhTgt *)D.tg, ntg, (const DhGlobal *)S.g,
                                   (const int32_t *)S.act, A, D.nzrecs, (const long long *)D.nzaoff);
                rc = fwi_fznz_submatrices_dev(c, ntg, D.nzrecs, A.acc, D.nzarena, (any_wl ? 2 * R.max_cap : R.max_cap) + 2, true, st);
                if (!rc) rc = fwi_fznz_segments_dev(c, y.grid_seg, S.segs, A.acc, S.so, d_ns, any_big, &S.g->any_big, D.nzrecs, D.nzarena, st);
            } else {
                rc = y.fz ? fwi_fz_segments_dev(c, y.grid_seg, S.segs, A.acc, S.so, d_ns, any_big, &S.g->any_big, st)
                          : fwi_mi_segments_dev(c, grid_mi, S.segs, A.acc, S.so, d_ns, st);
            }
            if (rc) return rc;
            if (timed(b, r)) (void)hipEventRecord(ev(q, 2 * r + 1), st);
            if ((rc = planfill((b * (unsigned)y.nb + (unsigned)r) % 16u == 0u))) return rc;  // the list of unfinished targets is compacted every 16 rounds
        }
        FW_HIP(c, hipGetLastError());
        FW_HIP(c, hipMemcpyAsync(R.hg + q, S.g, sizeof(DhGlobal), hipMemcpyDeviceToHost, st));
        FW_HIP(c, hipEventRecord(E.ev_end[q], st));
        return FW_OK;
    }
    // *done: the record of batch b says that every target has finished
    int retire_batch(unsigned b, int *done)
    {
        const int q = (int)(b & 1u);
        FW_HIP(c, hipEventSynchronize(E.ev_end[q]));
        const DhGlobal &rec = R.hg[q];
        for (int r = 0; r < y.nb; ++r) {
            if (rec.ns_ring[(b * (unsigned)y.nb + (unsigned)r) & 63u] == 0) continue;  // empty launch after the last round
            ++R.launches_n;
            if (!timed(b, r)) continue;
            float ms = 0.0f;
            FW_HIP(c, hipEventElapsedTime(&ms, ev(q, 2 * r), ev(q, 2 * r + 1)));
            R.timed_s += 1e-3 * (double)ms;
            ++R.timed_n;
            if (y.log_path) {
                const size_t idx = (size_t)b * (size_t)y.nb + (size_t)r;
                if (R.log_ms.size() <= idx) R.log_ms.resize(idx + 1, 0.0f);
                R.log_ms[idx] = ms;
            }
        }
        if (y.fz && c->P.max_k <= 3 && big_skipped[q] && rec.max_a > (unsigned)FW_TAB_A)  // the bound above failed: fail loudly
            return fw_fail(c, FW_ERR_DEVICE, "device rounds: an accepted list of %u entries met a batch without the in-lane kernel", rec.max_a);
        R.max_a_seen = std::max(R.max_a_seen, rec.max_a);
        R.max_ab_seen = std::max(R.max_ab_seen, rec.max_ab);
        n_act_bound = std::min(n_act_bound, rec.n_act);
        *done = rec.done != 0u;
        return FW_OK;
    }
    int run()
    {
        int rc = y.use_hp ? hp_stream() : FW_OK;
        if (rc) return rc;
        R.max_ab_seen = (unsigned)R.max_wl;  // before any record: all whitelisted neighbours are still to come
        unsigned b = 0;
        int done = 0;
        if (!(rc = planfill(true)))  // nothing to merge yet: creates the first jobs and the first launch (plan #0)
            rc = enqueue_batch(0);
        while (!rc) {
            if ((rc = enqueue_batch(b + 1))) break;   // keep the GPU fed ...
            if ((rc = retire_batch(b, &done))) break;  // ... while the host reads the previous batch's record
            ++b;
            if (done) {
                int d2 = 0;
                rc = retire_batch(b, &d2);  // the batch still in flight holds only no-op rounds
                break;
            }
            if (b > 250000u) {  // every round finishes at least one window: this is a logic error, not a workload
                rc = fw_fail(c, FW_ERR_DEVICE, "device HITON: no convergence after %u rounds", b * (unsigned)y.nb);
                break;
            }
        }
        if (rc) (void)hipStreamSynchronize(st);
        return rc;
    }
};

// FW_DH_LOG: one line per planned launch, appended to the file
static int dh_write_log(const DhRun &R)
{
    fw_ctx *c = R.c;
    std::vector<ulonglong2> lg(DH_LOG_CAP);
    DhGlobal fin{};
    FW_HIP(c, hipMemcpy(&fin, R.D.s.g, sizeof(DhGlobal), hipMemcpyDeviceToHost));
    FW_HIP(c, hipMemcpy(lg.data(), R.D.log, sizeof(ulonglong2) * DH_LOG_CAP, hipMemcpyDeviceToHost));
    long long n_tpc = 0, n_pc = 0;  // interleaving survivors / elimination survivors
    for (const DhTgt &x : R.tg) {
        n_tpc += x.ntpc;
        n_pc += x.npc;
    }
    if (FILE *f = fopen(R.y.log_path, "a")) {
        fprintf(f, "# targets %d rounds %u tpc %lld pc %lld\n", R.ntg, fin.rounds, n_tpc, n_pc);
        for (unsigned r = 0; r < fin.rounds && r < DH_LOG_CAP; ++r)
            fprintf(f, "%u %llu %llu %llu %.1f\n", r, lg[r].x, lg[r].y >> 32, lg[r].y & 0xffffffffull,
                    r < R.log_ms.size() ? 1e3 * (double)R.log_ms[r] : 0.0);
        fclose(f);
    }
    return FW_OK;
}

// per-target states and PC lists back to the host
static int dh_download(DhRun &R, std::vector<FwDhResult> &out, FwDhFlat &flat)
{
    fw_ctx *c = R.c;
    const size_t tot = R.tot;
    flat.key.resize(tot);
    flat.stat.resize(tot);
    flat.pval.resize(tot);
    // four copies enqueued on the chain's stream and one wait, instead of four blocking copies on the null stream.  The destinations
    // are pageable vectors: HIP stages such a copy and may block the host in the call, so this only takes the four synchronisations of
    // the null stream out; it was not measured alone (pinned destinations would be the next step)
    FW_HIP(c, hipMemcpyAsync(R.tg.data(), R.D.tg, sizeof(DhTgt) * R.ntg, hipMemcpyDeviceToHost, R.st));
    if (tot) {
        FW_HIP(c, hipMemcpyAsync(flat.key.data(), R.A.pc_key, 4 * tot, hipMemcpyDeviceToHost, R.st));
        FW_HIP(c, hipMemcpyAsync(flat.stat.data(), R.A.pc_stat, 8 * tot, hipMemcpyDeviceToHost, R.st));
        FW_HIP(c, hipMemcpyAsync(flat.pval.data(), R.A.pc_p, 8 * tot, hipMemcpyDeviceToHost, R.st));
    }
    FW_HIP(c, hipStreamSynchronize(R.st));
    if (R.D.log)
        if (int rc = dh_write_log(R)) return rc;
    for (int t = 0; t < R.ntg; ++t) {
        const DhTgt &x = R.tg[t];
        if (x.phase != 2) return fw_fail(c, FW_ERR_DEVICE, "device HITON: target %d did not finish (phase %d)", x.T, x.phase);
        out[t].off = x.co;
        out[t].n = x.npc;
    }
    return FW_OK;
}

// FW_TRACE_HOST: chain statistics (the longest per-target sequences bound the pass from below) and the phase times
static void dh_trace_run(const DhRun &R, double t_setup, double t_rounds, double t_results)
{
    const std::vector<DhTgt> &tg = R.tg;
    const int chain = R.chain;
    unsigned long long mx_ref = 0, mx_calls = 0, tot_ref = 0, tot_calls = 0;
    int t_ref = -1, t_calls = -1;
    for (const DhTgt &x : tg) {
        tot_ref += x.c_ref;
        tot_calls += x.c_calls;
        if (x.c_ref > mx_ref) mx_ref = x.c_ref, t_ref = x.T;
        if (x.c_calls > mx_calls) mx_calls = x.c_calls, t_calls = x.T;
    }
    fprintf(stderr, "[fw] chain %d: tests %llu jobs %llu; most tests in one target %llu (T=%d), most jobs in one target %llu (T=%d)\n",
            chain, tot_ref, tot_calls, mx_ref, t_ref, mx_calls, t_calls);
    unsigned long long ev_all = 0, ev_short = 0;
    int na_max = 0;
    for (const DhTgt &x : tg) {
        ev_all += x.c_eval;
        ev_short += x.c_eval_short;
        na_max = std::max(na_max, x.na_max);
    }
    fprintf(stderr, "[fw] chain %d: executed tests %llu, of them in jobs with at most %d accepted variables %llu; longest accepted list %d\n",
            chain, ev_all, (int)FW_HK_A, ev_short, na_max);
    if (R.y.per_target) {  // the targets that finished last: when they were taken, how long they ran, what they ran
        unsigned int t0 = ~0u;
        for (const DhTgt &x : tg) t0 = std::min(t0, x.r_first0);
        std::vector<const DhTgt *> by_end;
        for (const DhTgt &x : tg) by_end.push_back(&x);
        std::sort(by_end.begin(), by_end.end(), [&](const DhTgt *a, const DhTgt *b) { return a->r_more0 - t0 > b->r_more0 - t0; });
        for (size_t i = 0; i < by_end.size() && i < 6; ++i) {
            const DhTgt *w = by_end[i];
            fprintf(stderr, "[fw]   finished at %.2f ms (taken at %.2f): T=%d, %d candidates, %d in PC, %llu jobs, %llu tests (%llu executed); "
                            "sequential prefixes %.2f ms, board phases %.2f ms (%llu jobs went to a board; %llu team rounds)\n",
                    1e-5 * (w->r_more0 - t0), 1e-5 * (w->r_first0 - t0), w->T, w->cap, w->npc, w->c_calls, w->c_ref, w->c_eval,
                    1e-5 * w->r_first1, 1e-5 * w->r_more1, w->c_eval_short & 0xffffffffull, w->c_eval_short >> 32);
        }
    } else {  // the target that was busy for the most rounds: where its rounds went
        const DhTgt *w = &tg[0];
        for (const DhTgt &x : tg)
            if (x.r_first0 + x.r_more0 + x.r_first1 + x.r_more1 > w->r_first0 + w->r_more0 + w->r_first1 + w->r_more1) w = &x;
        fprintf(stderr, "[fw] chain %d: longest-busy target T=%d: %d candidates, %d in TPC, %d in PC, %llu jobs; rounds: interleaving first windows %u, later windows %u; elimination first %u, later %u\n",
                chain, w->T, w->cap, w->ntpc, w->npc, w->c_calls, w->r_first0, w->r_more0, w->r_first1, w->r_more1);
    }
    fprintf(stderr, "[fw] chain %d: longest accepted list %u, accepted + whitelisted to come %u (most whitelisted neighbours of one target %d)\n",
            chain, R.max_a_seen, R.max_ab_seen, R.max_wl);
    fprintf(stderr, "[fw] device rounds chain %d: %d targets, set-up %.2f ms, rounds %.2f ms, results %.2f ms\n", chain, R.ntg,
            1e3 * t_setup, 1e3 * t_rounds, 1e3 * t_results);
}

// what the launches of a finished (or failed) run add to the context's counters: the kernels of every round of the segment kernel
// (the persistent kernel: itself) and `extra_kernels`, what the caller launched around them
static void dh_count_run(const DhRun &R, long extra_kernels)
{
    fw_ctx *c = R.c;
    std::lock_guard<std::mutex> lk(dh_cnt_mu);
    if (R.timed_n > 0) c->cnt.t_dev_subsets_s += R.timed_s * (double)R.launches_n / (double)R.timed_n;
    c->cnt.subsets_launches += R.launches_n + R.light_n;
    c->cnt.kernel_launches += (R.y.per_target ? R.launches_n : (R.y.nzk ? 7 : 4) * R.launches_n) + R.light_n + extra_kernels;
}

// Light targets (dh_fz_light_kernel): the largest level-0 degree the pre-pass of a run serves, 0: none.  Fisher-z on the Float32
// matrix with max_k <= 3 and no rejection log; everything else keeps the rounds.  At most FW_TAB_A / 2: a pool can hold every
// candidate twice (whitelist duplicates) and must still take the table variant of the segment body.  Read per call (the tests switch it
// inside a live process).  Default 32, by the sweep of profiles/r15_light_targets.txt
static int dh_light_deg(const fw_ctx *c, const DhPolicy &y)
{
    if (c->P.kind != FW_FZ || c->f64 || !c->d_cor || c->P.max_k < 1 || c->P.max_k > 3 || c->d_rej_run || y.per_target) return 0;
    return std::min(std::max(fw_knob_int(knob::FW_DH_LIGHT_DEG, 32), 0), FW_TAB_A / 2);
}

// The pre-pass in front of DhRounds, for the round loop and the slots of the schedule alike: one launch finishes the n_light light
// targets of the run (the kernel tells them from the others by the same rule, dh_is_light), so that DhRounds -- whose first step kernel
// finds them finished and whose first compaction drops them -- runs on what is left, or not at all.  R.D.tg, R.A (local matrices
// included) and R.P are in place; the launch goes to the run's stream, in front of its rounds.
static int dh_light_prepass(DhRun &R, int light_deg, int n_light)
{
    if (n_light == 0) return FW_OK;
    fw_ctx *c = R.c;
    double zscale = 0.0;
    if (int rc = fwi_fz_thresholds(c, R.st, &zscale)) return rc;
    hipLaunchKernelGGL(dh_fz_light_kernel, dim3((unsigned)R.ntg), dim3(256), 0, R.st, R.D.tg, R.ntg, light_deg, R.A, R.D.s.so, R.P,
                       (const float *)c->d_cor, c->P.p, zscale, (const double *)c->d_thr);
    FW_HIP(c, hipGetLastError());
    R.light_n = 1;
    return FW_OK;
}

// One round of targets on the device.  in: T ids, interleaving candidates and (sorted) whitelists per target;
// out: PC (keys, statistics, p-values) per target in insertion order.
int fwi_devhiton_run(fw_ctx *c, const std::vector<FwDhTarget> &in, std::vector<FwDhResult> &out, FwDhFlat &flat, int chain)
{
    const int ntg = (int)in.size();
    out.assign((size_t)ntg, FwDhResult{});
    if (ntg == 0) return FW_OK;
    static const bool trace_host = fw_trace_host();  // host-side phase times on stderr
    const double th0 = fwi_now_s();
    // chain > 0: a second (third, ...) instance running concurrently from its own host thread on its own stream / arena
    if (chain > 0 && !c->dh_stream[chain]) FW_HIP(c, hipStreamCreateWithFlags(&c->dh_stream[chain], hipStreamNonBlocking));
    DhRun R{c, chain, ntg, chain == 0 ? c->pb[0].stream : c->dh_stream[chain], trace_host, dh_policy(c, ntg)};
    dh_build_targets(R, in);
    int rc;
    if ((rc = dh_upload(R))) return rc;
    DhEvents E(R.st, 2 * 2 * DH_BATCH, 2);
    if (!E.ok) return fw_fail(c, FW_ERR_DEVICE, "device HITON: hipEventCreate failed");
    const double th1 = fwi_now_s();
    if (R.y.per_target) {
        rc = dh_run_persistent(R, E);
    } else {
        const int light_deg = dh_light_deg(c, R.y);
        int n_light = 0;
        for (const DhTgt &x : R.tg) n_light += dh_is_light(x.nb_n, x.cap, light_deg) ? 1 : 0;
        rc = dh_light_prepass(R, light_deg, n_light);
        if (!rc && n_light < ntg) rc = DhRounds(R, E).run();  // (a run of light targets alone: no round, no batch, no record to wait for)
    }
    dh_count_run(R, 0);
    if (rc) return rc;
    const double th2 = fwi_now_s();
    if ((rc = dh_download(R, out, flat))) return rc;
    if (trace_host) dh_trace_run(R, th1 - th0, th2 - th1, fwi_now_s() - th2);
    std::lock_guard<std::mutex> lk(dh_cnt_mu);
    for (const DhTgt &x : R.tg) {
        c->cnt.cond_tests_ref += (int64_t)x.c_ref;
        c->cnt.subsets_calls += (int64_t)x.c_calls;
        c->cnt.cond_tests_evaluated += (int64_t)x.c_eval;
        c->cnt.alg_bytes_subsets += x.c_alg;
    }
    return FW_OK;
}

// ---- what the two whole-schedule drivers share (fwi_devhiton_mi_schedule, fwi_devhiton_fz_schedule) ----

// the schedule: sched[0 .. nt) in rounds of R targets (learning.jl:97-98); round_of[v]: the round of variable v's own target, "never"
// where it has none
struct DhSchedPlan {
    int nt, R, nrounds;
    std::vector<int32_t> round_of;
    DhSchedPlan(const int32_t *sched, int nt_, int R_, int p) : nt(nt_), R(R_ <= 0 || R_ > nt_ ? nt_ : R_), nrounds((nt + R - 1) / R), round_of((size_t)p, 0x7fffffff)
    {
        for (int i = 0; i < nt; ++i) round_of[sched[i]] = i / R;
    }
    int first(int r) const { return r * R; }
    int count(int r) const { return std::min(nt, r * R + R) - r * R; }
};

// what lives for the whole schedule: every target's state, its lists at its level-0 offset nb_off[T] with its degree as capacity, the
// device-built whitelists' counts, the packed results
struct DhSchedState {
    DhTgt *tg;
    int32_t *round_of;
    unsigned int *wl_cnt;
    DhLists lists;
    int32_t *ot, *ou;  // packed results: target, neighbour, statistic, p
    double *os, *op;
    unsigned long long *tot;  // [0..4] integers, [5] the Float64 sum of algorithmic bytes
};
// acc_d1: accepted-list buffers per target (1 for the discrete kinds, look-ahead + 1 for Fisher-z)
static DhSchedState dh_sched_state_layout(DhArena &a, size_t nt, size_t p, size_t nnz, size_t acc_d1)
{
    DhSchedState b{};
    b.tg = a.take<DhTgt>(nt);
    b.round_of = a.take<int32_t>(p);
    b.wl_cnt = a.take<unsigned int>(p);
    b.lists = dh_lists_layout(a, nnz, acc_d1, nnz);
    b.ot = a.take<int32_t>(nnz, 4);
    b.ou = a.take<int32_t>(nnz, 4);
    b.os = a.take<double>(nnz, 8);
    b.op = a.take<double>(nnz, 8);
    b.tot = a.take<unsigned long long>(8);
    return b;
}

// Start of a schedule, on stream st: no result and no whitelist entry yet (a call leaves nothing behind for the next one), the round
// of every variable, and the state of every target (dh_sched_init_kernel; d_T: the targets in the order of S.tg, uploaded by the
// caller on the same stream).  The two memsets, the copy and the caller's own uploads are independent operations on one stream in
// front of the init kernel: since the schedules share this start, each enqueues them in another order than it did on its own.
static int dh_sched_begin(fw_ctx *c, hipStream_t st, const DhSchedState &S, const DhSchedPlan &pl, const int32_t *d_T, const int32_t *levels,
                          const long long *slot_tm, int wl_unsorted)
{
    const size_t p = pl.round_of.size();
    FW_HIP(c, hipMemsetAsync(S.tot, 0, 64, st));
    FW_HIP(c, hipMemsetAsync(S.wl_cnt, 0, 4 * p, st));
    FW_HIP(c, hipMemcpyAsync(S.round_of, pl.round_of.data(), 4 * p, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dh_sched_init_kernel, dim3((unsigned)((pl.nt + 255) / 256)), dim3(256), 0, st, S.tg, pl.nt, d_T, (const long long *)c->d_nb_off, levels,
                       slot_tm, wl_unsorted);
    FW_HIP(c, hipGetLastError());
    return FW_OK;
}

// after a round of targets tg[0 .. ntg): interleaved.jl:136-140, kept where a later round reads it (dh_wl_append_kernel)
static void dh_sched_append(fw_ctx *c, hipStream_t st, const DhSchedState &S, const DhTgt *tg, int ntg, int round)
{
    hipLaunchKernelGGL(dh_wl_append_kernel, dim3((unsigned)((ntg + 3) / 4)), dim3(256), 0, st, tg, ntg, (const int32_t *)S.lists.pc_key,
                       (const int32_t *)S.round_of, round, S.lists.wl, (const long long *)c->d_nb_off, S.wl_cnt);
}

// results of a schedule: packed on the device (dh_sched_pack_kernel, enqueued behind the last round on st) ...
static int dh_sched_pack(fw_ctx *c, hipStream_t st, const DhSchedState &S, int nt)
{
    hipLaunchKernelGGL(dh_sched_pack_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, (const DhTgt *)S.tg, nt, (const int32_t *)S.lists.pc_key,
                       (const double *)S.lists.pc_stat, (const double *)S.lists.pc_p, S.ot, S.ou, S.os, S.op, S.tot, (double *)(S.tot + 5));
    FW_HIP(c, hipGetLastError());
    return FW_OK;
}
// ... the totals read back (with whatever the caller enqueued behind the pack kernel: the stream is idle on return) ...
static int dh_sched_totals(fw_ctx *c, hipStream_t st, const DhSchedState &S, unsigned long long (&htot)[8])
{
    FW_HIP(c, hipMemcpyAsync(htot, S.tot, 64, hipMemcpyDeviceToHost, st));
    FW_HIP(c, hipStreamSynchronize(st));
    return FW_OK;
}
// ... and, once they are believed, one small download: (target, neighbour, statistic, p) appended to `all`, a target's entries together,
// in PC insertion order.  The destinations are pageable: staged copies that may block in the call -- 0.9 ms for cfg3's 3.6 MB.
static int dh_sched_finish(fw_ctx *c, hipStream_t st, const DhSchedState &S, const unsigned long long (&htot)[8], size_t nnz, FwDirected &all)
{
    if (htot[4]) return fw_fail(c, FW_ERR_DEVICE, "device schedule: %llu targets did not finish", htot[4]);
    const size_t nres = (size_t)htot[0], at0 = all.size();
    if (nres > nnz) return fw_fail(c, FW_ERR_DEVICE, "device schedule: %zu result entries for %zu level-0 entries", nres, nnz);
    all.resize(at0 + nres);
    if (nres) {
        FW_HIP(c, hipMemcpyAsync(all.t.data() + at0, S.ot, 4 * nres, hipMemcpyDeviceToHost, st));
        FW_HIP(c, hipMemcpyAsync(all.u.data() + at0, S.ou, 4 * nres, hipMemcpyDeviceToHost, st));
        FW_HIP(c, hipMemcpyAsync(all.s.data() + at0, S.os, 8 * nres, hipMemcpyDeviceToHost, st));
        FW_HIP(c, hipMemcpyAsync(all.p.data() + at0, S.op, 8 * nres, hipMemcpyDeviceToHost, st));
        FW_HIP(c, hipStreamSynchronize(st));
    }
    c->cnt.cond_tests_ref += (int64_t)htot[1];
    c->cnt.subsets_calls += (int64_t)htot[2];
    c->cnt.cond_tests_evaluated += (int64_t)htot[3];
    double alg;
    memcpy(&alg, &htot[5], sizeof(double));
    c->cnt.alg_bytes_subsets += alg;
    return FW_OK;
}

// ---- the whole feed-forward schedule of the discrete kinds (fwi_devhiton_mi_schedule) ----

struct DhSchedSizes {
    size_t nt, p, nnz, nrounds;
};
struct DhSchedBufs {
    DhSchedState S;
    int32_t *sched, *order;
    MiQueue *mq;  // one per round
    MiBoard *boards;
    FwSegOut *mres;
    int32_t *bacc;
};
static DhSchedBufs dh_sched_layout(DhArena &a, const DhSchedSizes &z)
{
    DhSchedBufs b{};
    b.S = dh_sched_state_layout(a, z.nt, z.p, z.nnz, 1);
    b.sched = a.take<int32_t>(z.nt);
    b.order = a.take<int32_t>(z.nt);
    b.mq = a.take<MiQueue>(z.nrounds);
    b.boards = a.take<MiBoard>(MI_BOARD_CAP);
    b.mres = a.take<FwSegOut>(MI_REC_CAP);
    b.bacc = a.take<int32_t>(MI_BACC_CAP);
    return b;
}

// The WHOLE feed-forward schedule of the discrete kinds on the device (r05; one GPU, no exchange between the rounds).  r02-r04 ran one
// persistent launch per round with the host in between: download the round's PC lists, update the running graph, build the next round's
// targets and whitelists, upload -- cfg4: ~1.4 ms per round besides the kernel (ten rounds) plus 5 ms before the first one, for nine
// launches of 1-3 ms each.  Here the state of every target of the schedule is built on the device from the level-0 CSR
// (dh_sched_init_kernel), the whitelists grow on the device between two launches (dh_wl_append_kernel: interleaved.jl:136-140 kept where a
// later round reads it), and the launches of all rounds are enqueued back to back; the host reads the results once.  Semantics per
// round are those of fwi_devhiton_run (same kernel, same per-round order and team size).  sched[0 .. nt): the targets in schedule order
// (learning.jl:97-98); rounds of R targets.  Appends (target, neighbour, statistic, p): a target's entries together, in PC insertion order.
int fwi_devhiton_mi_schedule(fw_ctx *c, const int32_t *sched, int nt, int R, bool feed_forward, FwDirected &all)
{
    if (nt == 0) return FW_OK;
    if (!c->d_cand || !c->d_nb_idx) return fw_fail(c, FW_ERR_STATE, "device schedule: the level-0 lists are not on the device");
    static const bool trace_host = fw_trace_host();
    const double th0 = fwi_now_s();
    hipStream_t st = c->pb[0].stream;
    const int p = c->P.p;
    const size_t nnz = (size_t)c->nb_off[p];
    const DhSchedPlan pl(sched, nt, R, p);
    const int nrounds = pl.nrounds;
    // ---- host: per-round order and team sizes ----
    std::vector<int32_t> order((size_t)nt), deg((size_t)nt);
    std::vector<unsigned> team((size_t)nrounds, 0u);
    // (the degrees from an array filled once: read from the level-0 offsets inside the sort's comparison they cost cfg4's 50 020 targets
    // 0.6 ms of set-up, 0.93 -> 1.56 ms -- the set-up time of FW_TRACE_HOST is where a host regression of this driver shows)
    for (int i = 0; i < nt; ++i) deg[i] = (int32_t)(c->nb_off[sched[i] + 1] - c->nb_off[sched[i]]);
    for (int r = 0; r < nrounds; ++r) {
        const int32_t *d = deg.data() + pl.first(r);
        team[r] = dh_heaviest_first(order.data() + pl.first(r), pl.count(r), [&](int32_t i) { return d[i]; });
    }
    // ---- device arena ----
    DhSchedBufs D;
    if (int rc = dh_arena_reserve(c, c->d_dh[0], dh_sched_layout, DhSchedSizes{(size_t)nt, (size_t)p, nnz, (size_t)nrounds}, &D)) return rc;
    DhArrays A = dh_arrays(c, c->d_cand, D.S.lists, DhLevel0{});
    A.wl_cnt = feed_forward ? D.S.wl_cnt : nullptr;
    FW_HIP(c, hipMemcpyAsync(D.sched, sched, 4 * (size_t)nt, hipMemcpyHostToDevice, st));
    FW_HIP(c, hipMemcpyAsync(D.order, order.data(), 4 * (size_t)nt, hipMemcpyHostToDevice, st));
    FW_HIP(c, hipMemsetAsync(D.mq, 0, sizeof(MiQueue) * (size_t)nrounds, st));
    if (int rc = dh_sched_begin(c, st, D.S, pl, D.sched, (const int32_t *)c->d_levels, nullptr, 1)) return rc;
    const DhParams P = dh_make_params(c, pl.R, 0, 0);
    DhEvents E(st, 2, 0);
    if (!E.ok) return fw_fail(c, FW_ERR_DEVICE, "device schedule: hipEventCreate failed");
    const double th1 = fwi_now_s();
    FW_HIP(c, hipEventRecord(E.ev[0], st));
    std::vector<unsigned> grids((size_t)nrounds, 0u);
    for (int r = 0; r < nrounds; ++r) {
        const int r0 = pl.first(r), ntg = pl.count(r);
        FW_HIP(c, hipMemsetAsync(D.boards, 0, sizeof(MiBoard) * MI_BOARD_CAP, st));  // ready flags, claimed / finished counts
        grids[r] = dh_mi_launch(c, st, D.S.tg + r0, ntg, (const int32_t *)(D.order + r0), A, P, team[r], trace_host, D.mq + r, D.boards, D.mres, D.bacc);
        if (feed_forward && r + 1 < nrounds) dh_sched_append(c, st, D.S, D.S.tg + r0, ntg, r);
    }
    FW_HIP(c, hipGetLastError());
    FW_HIP(c, hipEventRecord(E.ev[1], st));
    // ---- results ----
    if (int rc = dh_sched_pack(c, st, D.S, nt)) return rc;
    std::vector<MiQueue> hq((size_t)nrounds);
    FW_HIP(c, hipMemcpyAsync(hq.data(), D.mq, sizeof(MiQueue) * (size_t)nrounds, hipMemcpyDeviceToHost, st));
    unsigned long long htot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (int rc = dh_sched_totals(c, st, D.S, htot)) return rc;
    const double th2 = fwi_now_s();
    for (int r = 0; r < nrounds; ++r)  // (a watchdog leaves targets unfinished: its message first)
        if (int rc = dh_mi_check(c, hq[r], grids[r], r, pl.count(r), trace_host)) return rc;
    float ms = 0.0f;
    FW_HIP(c, hipEventElapsedTime(&ms, E.ev[0], E.ev[1]));
    if (int rc = dh_sched_finish(c, st, D.S, htot, nnz, all)) return rc;
    c->cnt.t_dev_subsets_s += 1e-3 * (double)ms;
    c->cnt.subsets_launches += nrounds;
    c->cnt.kernel_launches += 2 * nrounds + 1;
    if (trace_host)
        fprintf(stderr, "[fw] device schedule: %d targets in %d rounds, set-up %.2f ms, launches + download %.2f ms (kernels %.2f ms), results %.2f ms\n", nt, nrounds,
                1e3 * (th1 - th0), 1e3 * (th2 - th1), (double)ms, 1e3 * (fwi_now_s() - th2));
    return FW_OK;
}

// ---- the whole feed-forward schedule of Fisher-z (fwi_devhiton_fz_schedule) ----

struct DhFzChainSizes {
    size_t ntg, max_ns, tm_floats;  // the largest round of the chain, each
};
struct DhFzSizes {
    size_t nt, p, nnz, d1, nslots;
    int K;
    DhFzChainSizes ch[FW_DH_MAX_CHAINS];
};
struct DhFzBufs {
    DhSchedState S;  // (S.tg: every target of the schedule, in slot order)
    int32_t *slot_T;
    long long *slot_tm;
    unsigned int *wl_max;                 // one word per (round, chain)
    DhRoundScratch ch[FW_DH_MAX_CHAINS];  // a chain's scratch: reserved once, for its largest round
};
static DhFzBufs dh_fz_layout(DhArena &a, const DhFzSizes &z)
{
    DhFzBufs b{};
    b.S = dh_sched_state_layout(a, z.nt, z.p, z.nnz, z.d1);
    b.slot_T = a.take<int32_t>(z.nt);
    b.slot_tm = a.take<long long>(z.nt);
    b.wl_max = a.take<unsigned int>(z.nslots);
    for (int q = 0; q < z.K; ++q) b.ch[q] = dh_scratch_layout(a, z.ch[q].ntg, z.ch[q].max_ns, z.ch[q].tm_floats);
    return b;
}

// where the host threads of the chains meet between two rounds of targets; an error of any chain ends the schedule for all of them
struct DhFzBarrier {
    std::mutex m;
    std::condition_variable cv;
    int n, waiting = 0, rc = FW_OK;
    unsigned gen = 0;
    explicit DhFzBarrier(int k) : n(k) {}
    int arrive(int my_rc)
    {
        std::unique_lock<std::mutex> lk(m);
        if (my_rc && !rc) rc = my_rc;
        const unsigned g = gen;
        if (++waiting == n) {
            waiting = 0;
            ++gen;
            cv.notify_all();
        } else {
            cv.wait(lk, [&] { return gen != g; });
        }
        return rc;
    }
};

// a chain's share of one round of the schedule
struct DhFzSlot {
    int base = 0, ntg = 0, max_cap = 0;
    int n_light = 0;  // targets of the slot that the pre-pass finishes (dh_light_prepass)
    unsigned max_ns = 0;
    size_t tm_floats = 0;
};

// The WHOLE feed-forward schedule of Fisher-z on the device (one GPU, no exchange between the rounds): what fwi_devhiton_mi_schedule
// does for the discrete kinds.  The round loop (fw_hiton.cpp: run_rounds) paid per round of targets: whitelists from the host's running
// graph, one FwDhTarget per target, a thread per chain, dh_build_targets + dh_upload, 66 events made and destroyed, four downloads, one
// push per result entry and the running graph's update -- 0.8 ms of host time around ~1.1 ms of device rounds in each of cfg3's nine
// light rounds (profiles/r14_fz_device_schedule.txt).  Here the host computes the layout of every round once (slots: round, chain, index
// in the chain; the round loop's deal, its per-chain policy and its layout rule: dh_tm_off, dh_max_ns), the state of every target is
// built on the device (dh_sched_init_kernel), the whitelists grow on the device (dh_wl_append_kernel, sorted at the start of the round
// that reads them: dh_fz_round_begin_kernel), and the chains' host threads live for the whole schedule.  Level-synchronous as before: a
// chain starts round r + 1 when every chain has retired round r (DhFzBarrier) and its stream has waited for the other chains' appends
// (events).  Per round and chain the host reads ONE word (the longest whitelist: DhRounds needs the exact bound, see enqueue_batch)
// besides the batch records.  Results: packed on the device, one download.  sched[0 .. nt): the targets in schedule order, rounds of R.
int fwi_devhiton_fz_schedule(fw_ctx *c, const int32_t *sched, int nt, int R, bool feed_forward, FwDirected &all)
{
    if (nt == 0) return FW_OK;
    if (!c->d_cand || !c->d_nb_idx || !c->d_nb_off) return fw_fail(c, FW_ERR_STATE, "device schedule: the level-0 lists are not on the device");
    static const bool trace_host = fw_trace_host();
    const double th0 = fwi_now_s();
    const int p = c->P.p;
    const size_t nnz = (size_t)c->nb_off[p];
    const DhSchedPlan pl(sched, nt, R, p);
    const int nrounds = pl.nrounds;
    // ---- host, once: the slots of every round (deal_chains order), their DhTgt offsets and sizes ----
    int K = 1;
    for (int r = 0; r < nrounds; ++r) K = std::max(K, fwi_chain_count(c, (size_t)pl.count(r)));
    std::vector<DhFzSlot> slots((size_t)nrounds * (size_t)K);
    std::vector<int32_t> slot_T((size_t)nt);
    std::vector<long long> slot_tm((size_t)nt);
    DhFzSizes z{(size_t)nt, (size_t)p, nnz, 0, (size_t)nrounds * (size_t)K, K, {}};
    {
        std::vector<int> chain_of;
        std::vector<size_t> chain_idx;
        for (int r = 0; r < nrounds; ++r) {
            const int r0 = pl.first(r), n = pl.count(r);
            const int Kr = fwi_chain_count(c, (size_t)n);
            fwi_deal_chains((size_t)n, Kr, chain_of, chain_idx);
            DhFzSlot *s = &slots[(size_t)r * (size_t)K];
            for (int i = 0; i < n; ++i) ++s[chain_of[i]].ntg;
            for (int q = 0, base = r0; q < K; ++q) {
                s[q].base = base;
                base += s[q].ntg;
            }
            for (int i = 0; i < n; ++i) slot_T[(size_t)s[chain_of[i]].base + chain_idx[i]] = sched[r0 + i];
            for (int q = 0; q < K; ++q) {
                if (s[q].ntg == 0) continue;
                const DhPolicy y = dh_policy(c, s[q].ntg);
                const int light_deg = dh_light_deg(c, y);
                z.d1 = (size_t)y.spec_depth + 1;
                for (int t = 0; t < s[q].ntg; ++t) {
                    const int T = slot_T[(size_t)(s[q].base + t)];
                    const int deg = (int)(c->nb_off[T + 1] - c->nb_off[T]);
                    s[q].max_cap = std::max(s[q].max_cap, deg);
                    s[q].n_light += dh_is_light(deg, deg, light_deg) ? 1 : 0;  // (dh_sched_init_kernel: capacity = degree)
                    slot_tm[(size_t)(s[q].base + t)] = dh_tm_off(c, y, deg, s[q].tm_floats);
                }
                s[q].max_ns = dh_max_ns(y, s[q].ntg);
                z.ch[q].ntg = std::max(z.ch[q].ntg, (size_t)s[q].ntg);
                z.ch[q].max_ns = std::max(z.ch[q].max_ns, (size_t)s[q].max_ns);
                z.ch[q].tm_floats = std::max(z.ch[q].tm_floats, s[q].tm_floats);
            }
        }
    }
    // ---- device arena (reserved once: growing it mid-schedule would synchronise the device under the other chain), streams, events ----
    DhFzBufs D;
    if (int rc = dh_arena_reserve(c, c->d_dh[0], dh_fz_layout, z, &D)) return rc;
    hipStream_t sts[FW_DH_MAX_CHAINS];
    for (int q = 0; q < K; ++q) {
        if (q > 0 && !c->dh_stream[q]) FW_HIP(c, hipStreamCreateWithFlags(&c->dh_stream[q], hipStreamNonBlocking));
        sts[q] = q == 0 ? c->pb[0].stream : c->dh_stream[q];
        if (int rc = fw_pin_reserve(c, c->h_dh[q], 4096)) return rc;
    }
    static_assert(2 * sizeof(DhGlobal) <= 3072, "the pinned page holds two batch records and, at byte 3072, the whitelist word");
    hipStream_t st = sts[0];
    DhEvents X(st, 0, 3 * K);  // ev_end[q * 3 + 0 / 1]: chain q's round r (r & 1) and its appends are done; [q * 3 + 2]: the whitelist word
    if (!X.ok) return fw_fail(c, FW_ERR_DEVICE, "device schedule: hipEventCreate failed");
    const DhArrays A = dh_arrays(c, c->d_cand, D.S.lists, DhLevel0{});  // (tmat: per chain and round)
    FW_HIP(c, hipMemsetAsync(D.wl_max, 0, 4 * z.nslots, st));
    FW_HIP(c, hipMemcpyAsync(D.slot_T, slot_T.data(), 4 * (size_t)nt, hipMemcpyHostToDevice, st));
    FW_HIP(c, hipMemcpyAsync(D.slot_tm, slot_tm.data(), 8 * (size_t)nt, hipMemcpyHostToDevice, st));
    if (int rc = dh_sched_begin(c, st, D.S, pl, D.slot_T, nullptr, D.slot_tm, 0)) return rc;
    for (int q = 1; q < K; ++q) {  // the other chains' streams start behind the set-up
        FW_HIP(c, hipEventRecord(X.ev_end[(size_t)q * 3], st));
        FW_HIP(c, hipStreamWaitEvent(sts[q], X.ev_end[(size_t)q * 3], 0));
    }
    const double th1 = fwi_now_s();
    // ---- the rounds: one host thread per chain for the whole schedule ----
    DhFzBarrier bar(K);
    std::vector<double> t_start((size_t)nrounds, 0.0);
    auto chain_round = [&](int q, int r, DhEvents &E) -> int {
        const DhFzSlot &s = slots[(size_t)r * (size_t)K + (size_t)q];
        hipStream_t sq = sts[q];
        if (r > 0)
            for (int o = 0; o < K; ++o)
                if (o != q) FW_HIP(c, hipStreamWaitEvent(sq, X.ev_end[(size_t)o * 3 + (size_t)((r - 1) & 1)], 0));
        if (q == 0) t_start[(size_t)r] = fwi_now_s() - th0;
        DhRun Rn{c, q, s.ntg, sq, trace_host, dh_policy(c, s.ntg)};
        Rn.use_devc = true;
        Rn.dev_wl = true;
        Rn.max_cap = s.max_cap;
        Rn.max_ns = s.max_ns;
        Rn.tm_floats = s.tm_floats;
        Rn.D.tg = D.S.tg + s.base;
        Rn.D.s = D.ch[q];
        if (!s.tm_floats) Rn.D.s.tmat = nullptr;  // (the chain's block is sized for its largest round)
        const DhRoundScratch &cb = Rn.D.s;
        Rn.A = A;
        Rn.A.tmat = cb.tmat;
        Rn.hg = (DhGlobal *)c->h_dh[q].ptr;
        memset(Rn.hg, 0, 2 * sizeof(DhGlobal));
        unsigned int *h_wl_max = (unsigned int *)((char *)c->h_dh[q].ptr + 3072);
        unsigned int *d_wl_max = D.wl_max + (size_t)r * (size_t)K + (size_t)q;
        hipLaunchKernelGGL(dh_fz_round_begin_kernel, dim3((unsigned)s.ntg), dim3(256), 0, sq, Rn.D.tg, s.ntg, (const unsigned int *)D.S.wl_cnt, D.S.lists.wl,
                           cb.g, cb.seg0, cb.act, d_wl_max);
        FW_HIP(c, hipGetLastError());
        // a slot of light targets alone never enters DhRounds: no batch, and no whitelist word, which only DhRounds' in-lane bound reads
        const bool rounds = s.n_light < s.ntg;
        if (rounds && feed_forward && r > 0) {
            FW_HIP(c, hipMemcpyAsync(h_wl_max, d_wl_max, sizeof(unsigned int), hipMemcpyDeviceToHost, sq));
            FW_HIP(c, hipEventRecord(X.ev_end[(size_t)q * 3 + 2], sq));
        }
        if (cb.tmat) {
            hipLaunchKernelGGL(dh_tmat_build_kernel, dim3((unsigned)s.ntg, 8u), dim3(256), 0, sq, (const DhTgt *)Rn.D.tg, s.ntg, A.nb_idx,
                               (const float *)c->d_cor, p, cb.tmat);
            FW_HIP(c, hipGetLastError());
        }
        Rn.P = dh_make_params(c, s.ntg, Rn.y.spec_depth, Rn.y.spec0_depth);
        int rc = dh_light_prepass(Rn, dh_light_deg(c, Rn.y), s.n_light);
        if (!rc && rounds && feed_forward && r > 0) {  // the exact longest whitelist, before the round's first batch is enqueued
            FW_HIP(c, hipEventSynchronize(X.ev_end[(size_t)q * 3 + 2]));
            Rn.max_wl = (int)*h_wl_max;
        }
        if (!rc && rounds) rc = DhRounds(Rn, E).run();
        const bool append = !rc && feed_forward && r + 1 < nrounds;
        // besides the kernels of every round of the segment kernel, what this round of targets launches: the round-begin kernel, the
        // local matrices and the append where they run
        dh_count_run(Rn, 1 + (cb.tmat ? 1 : 0) + (append ? 1 : 0));
        if (rc) return rc;
        if (append) {
            dh_sched_append(c, sq, D.S, Rn.D.tg, s.ntg, r);
            FW_HIP(c, hipGetLastError());
        }
        return FW_OK;
    };
    auto chain_body = [&](int q) {
        DhEvents E(sts[q], 2 * 2 * DH_BATCH, 2);  // once per chain and schedule (its destructor synchronises the chain's stream)
        int rc = E.ok ? FW_OK : fw_fail(c, FW_ERR_DEVICE, "device schedule: hipEventCreate failed");
        for (int r = 0; r < nrounds; ++r) {
            if (!rc && slots[(size_t)r * (size_t)K + (size_t)q].ntg > 0) rc = chain_round(q, r, E);
            if (!rc && hipEventRecord(X.ev_end[(size_t)q * 3 + (size_t)(r & 1)], sts[q]) != hipSuccess)
                rc = fw_fail(c, FW_ERR_DEVICE, "device schedule: hipEventRecord failed");
            if ((rc = bar.arrive(rc))) break;  // (every chain leaves at the same barrier)
        }
    };
    {
        std::vector<std::thread> th;
        for (int q = 1; q < K; ++q)
            th.emplace_back([&, q] {
                (void)hipSetDevice(c->P.device);
                chain_body(q);
            });
        chain_body(0);
        for (std::thread &t : th) t.join();
    }
    if (bar.rc) return bar.rc;
    const double th2 = fwi_now_s();
    // ---- results (every chain has retired its last batch and synchronised its stream: the device is idle) ----
    if (int rc = dh_sched_pack(c, st, D.S, nt)) return rc;
    unsigned long long htot[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (int rc = dh_sched_totals(c, st, D.S, htot)) return rc;
    if (int rc = dh_sched_finish(c, st, D.S, htot, nnz, all)) return rc;
    c->cnt.kernel_launches += 2;  // dh_sched_init_kernel, dh_sched_pack_kernel
    if (trace_host) {
        fprintf(stderr, "[fw] fz device schedule: %d targets in %d rounds on %d chains, set-up %.2f ms, rounds %.2f ms, results %.2f ms; rounds start at", nt,
                nrounds, K, 1e3 * (th1 - th0), 1e3 * (th2 - th1), 1e3 * (fwi_now_s() - th2));
        for (int r = 0; r < nrounds; ++r) fprintf(stderr, " %.2f", 1e3 * t_start[(size_t)r]);
        fprintf(stderr, " ms\n");
    }
    return FW_OK;
}
