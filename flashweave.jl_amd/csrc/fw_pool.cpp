// The host job pool: progressive, segment-parallel evaluation of test_subsets jobs.  It serves fw_test_subsets_batch and every path the
// device rounds do not (max_k 6-7, recursive_pcor = 0, Float64, generic discrete data, small rounds, FW_HOST_HITON=1).  The records and
// the pure rules -- enumeration size, windows, segment length, growth, merge, advance -- are in fw_pool_host.h; here are the stages
// that touch the context: staging buffers, arenas, the segment back-ends and the streams.
//
// One window of every live job = one kernel launch on the pool's own stream.  fwi_pool_launch only enqueues; fwi_pool_collect waits
// for it and merges.  Two pools can therefore overlap: the host merges / re-posts one while the GPU evaluates the other.
#include <algorithm>

#include "fw_internal.h"

static bool pool_no_power(const fw_ctx *c) { return c->P.kind == FW_FZ && c->P.n < c->n_obs_min_eff; }

static void no_power_result(const fw_ctx *c, const int32_t *acc, int a, FwJobOut &o)
{
    // tests.jl:254-262: every test lacks power -> the first one is returned (0, 1, 0, false)
    o = FwJobOut{};
    o.stat = 0.0;
    o.pval = 1.0;
    o.num_tests = 1;
    o.evaluated = 0;
    o.status = FW_SUBSETS_STOPPED;
    const int s = std::min<int>(c->P.max_k, a);
    o.n_zs = s;
    for (int q = 0; q < s; ++q) o.zs[q] = acc[q];
}

int fwi_pool_add(fw_ctx *c, FwPool &pool, int32_t X, int32_t Y, const int32_t *acc, int a, int64_t tag)
{
    static const uint64_t w0_big = fw_knob_u64(knob::FW_W0_BIG, 16384ull);
    FwPoolJob j;
    j.X = X;
    j.Y = Y;
    j.tag = tag;
    j.acc.assign(acc, acc + a);
    j.N = fw_pool_enum_size(a, c->P.max_k, c->P.max_tests);
    j.width = fw_pool_first_window(c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ, a, w0_big);
    pool.live.push_back(std::move(j));
    return FW_OK;
}

static void finish_job(const fw_ctx *c, FwPoolJob &j, bool want_zs)
{
    j.done = true;
    j.out.n_zs = 0;
    if (!want_zs || j.no_zs) return;  // the HITON driver never looks at the conditioning set of the returned result
    int s = 0, pos[FW_MAX_K] = {0};
    fw_pool_unrank(j.best_rank, (int)j.acc.size(), c->P.max_k, &s, pos);  // conditioning set of the returned result
    j.out.n_zs = s;
    for (int q = 0; q < FW_MAX_K; ++q) j.out.zs[q] = q < s ? j.acc[pos[q]] : 0;
}

// ---- launch ------------------------------------------------------------------------------------------
// What the stages of one fwi_pool_launch hand on
struct PoolLaunch {
    bool stream = false;  // FW_FZ, recursive_pcor = 0: one wavefront per test on the sample columns (fw_fzs.hip)
    bool fz = false;      // one lane per test on a correlation matrix
    bool nzs = false;     // FW_FZ_NZ
    size_t n_launch = 0, acc_total = 0;  // launched jobs and the ints of their accepted lists
    uint64_t seglen = 0;
    size_t ns = 0, ns_tab = 0;  // segments; of them in front, for the table kernel
    size_t new_ints = 0;        // accepted-list ints this launch may have to stage
    size_t staged = 0;          // ... and did
    size_t arena_floats = 0;    // elements of the job-matrix arena the launch addresses
    FwSeg *segs = nullptr;      // staging (pinned): the segment records, behind them the accepted lists
    int32_t *hacc = nullptr;
    FwSegOut *dout = nullptr;   // where the kernels write their records: pinned host memory, or device memory under FW_ZC_OUT=0
};

// jobs whose owner's accepted set has changed since they were posted
static void pool_drop_stale(fw_ctx *c, FwPool &pool)
{
    if (!pool.owner_epoch) return;
    size_t w = 0;
    for (size_t ji = 0; ji < pool.live.size(); ++ji) {
        FwPoolJob &j = pool.live[ji];
        if (j.epoch != (*pool.owner_epoch)[(size_t)j.tag]) {
            pool.dropped_evaluated += j.out.evaluated;
            pool.dropped_alg_bytes += fwi_alg_bytes(c, (int)j.acc.size(), j.out.evaluated);
            continue;
        }
        if (w != ji) pool.live[w] = std::move(j);
        ++w;
    }
    pool.live.resize(w);
}

// window of every live job that is not on hold, then a segment length that yields a few thousand workgroups
static void pool_plan(fw_ctx *c, FwPool &pool, PoolLaunch &L)
{
    static const uint64_t seg_target = fw_seg_target();
    L.stream = c->P.kind == FW_FZ && !c->P.recursive_pcor;
    L.fz = (c->P.kind == FW_FZ || c->P.kind == FW_FZ_NZ) && !L.stream;
    L.nzs = c->P.kind == FW_FZ_NZ;
    // job matrices are kept across the rounds of this pool (ctx->d_arena): a new pool, or an arena another pool used, starts empty
    if (L.stream && (pool.gram_epoch == 0 || pool.gram_epoch != c->gram_epoch || pool.gram_top * sizeof(double) > ((size_t)4 << 30))) {
        pool.gram_epoch = ++c->gram_epoch;
        pool.gram_top = 0;
    }
    uint64_t total = 0;
    for (FwPoolJob &j : pool.live) {
        j.launched = !j.hold;
        if (!j.launched) continue;
        ++L.n_launch;
        total += fw_pool_window(j.next, j.width, j.N);
        L.acc_total += j.acc.size();
    }
    pool.launched_ranks = total;
    if (L.n_launch == 0) return;
    L.seglen = fw_pool_seglen(total, L.fz, seg_target);
    for (const FwPoolJob &j : pool.live)
        if (j.launched) L.ns += (size_t)fw_pool_nsegs(fw_pool_window(j.next, j.width, j.N), L.seglen);
}

// Accepted lists live in a device arena for as long as their job does: a job uploads its list once, with its first window, not with
// every window (at cfg3 the lists of ~1500 live jobs are ~1 MB per round).  The arena is a bump allocator; when it is full every live
// job is re-staged from offset 0.
static int pool_acc_arena(fw_ctx *c, FwPool &pool, FwPoolBuf &pb, PoolLaunch &L)
{
    for (const FwPoolJob &j : pool.live)
        if (j.launched && j.acc_dev_off < 0) L.new_ints += j.acc.size();
    if (pool.arena_top + L.new_ints > pb.d_acc.cap / sizeof(int32_t) || pool.arena_top == 0) {
        size_t live_ints = 0;
        for (FwPoolJob &j : pool.live) {
            j.acc_dev_off = -1;
            live_ints += j.acc.size();
        }
        if (int rc = fw_dev_reserve(c, pb.d_acc, std::max<size_t>(4 * live_ints, (size_t)1 << 20) * sizeof(int32_t))) return rc;
        pool.arena_top = 0;
        L.new_ints = L.acc_total;
    }
    return FW_OK;
}

// Results: one record per workgroup, written straight into pinned host memory (posted PCIe writes) -- saves the device-to-host copy
// of every round; FW_ZC_OUT=0 stages them through device memory instead (profiling knob)
static int pool_reserve_staging(fw_ctx *c, FwPoolBuf &pb, PoolLaunch &L)
{
    static const bool zc_out = fw_knob_on(knob::FW_ZC_OUT);
    const size_t in_bytes = L.ns * sizeof(FwSeg) + std::max<size_t>(L.new_ints, 1) * sizeof(int32_t);
    if (int rc = fw_pin_reserve(c, pb.h_in, in_bytes)) return rc;
    if (int rc = fw_pin_reserve(c, pb.h_out, L.ns * sizeof(FwSegOut))) return rc;
    if (int rc = fw_dev_reserve(c, pb.d_in, L.ns * sizeof(FwSeg))) return rc;
    if (!zc_out)
        if (int rc = fw_dev_reserve(c, pb.d_out, L.ns * sizeof(FwSegOut))) return rc;
    L.dout = zc_out ? (FwSegOut *)pb.h_out.ptr : (FwSegOut *)pb.d_out.ptr;
    L.segs = (FwSeg *)pb.h_in.ptr;
    L.hacc = (int32_t *)((char *)pb.h_in.ptr + L.ns * sizeof(FwSeg));
    return FW_OK;
}

static void count_gram_job(fw_ctx *c, const FwNzJob &r)  // (the job-matrix form's own algorithmic unit, fw_counters)
{
    c->cnt.gram_jobs += 1;
    c->cnt.gram_alg_bytes += (double)r.m * (double)c->P.n * 4.0;
    c->cnt.gram_alg_flops += 2.0 * (double)c->P.n * 0.5 * (double)r.m * (double)(r.m - 1);
}

// Segment records of every launched job (pool.seg_job: their jobs) and, for fz_nz and recursive_pcor = 0, one FwNzJob per launched job
// in pool.nzrecs (FwSeg::pad indexes it).  fz / fz_nz: the segments of jobs with short accepted lists come first (table kernels), so
// the jobs are walked in two passes and neither segments nor records follow pool.live order.
static void pool_build_records(fw_ctx *c, FwPool &pool, PoolLaunch &L)
{
    static const bool no_tab = fw_knob_set(knob::FW_NO_TAB);  // profiling knob: force the in-lane caching kernel
    const bool no_hk = fw_no_hk();   // profiling / test knob: generic size-4/5 kernel for every job
    const bool hk = c->P.max_k > 3;  // max_k 4-5: level-2 table kernel up to FW_HK_A accepted variables (plain fz only); else the LDS table up to FW_TAB_A
    const bool split = L.fz && !no_tab && (!hk || (c->P.kind == FW_FZ && !L.stream && !no_hk));
    const size_t tab_a = hk ? (size_t)FW_HK_A : (size_t)FW_TAB_A;
    pool.seg_job.resize(L.ns);
    pool.nzrecs.clear();
    size_t si = 0;
    for (int pass = 0; pass < (split ? 2 : 1); ++pass) {
        for (size_t ji = 0; ji < pool.live.size(); ++ji) {
            FwPoolJob &j = pool.live[ji];
            if (!j.launched) continue;
            if (split && (j.acc.size() <= tab_a) != (pass == 0)) continue;
            if (j.acc_dev_off < 0) {
                memcpy(L.hacc + L.staged, j.acc.data(), j.acc.size() * sizeof(int32_t));
                j.acc_dev_off = (int64_t)(pool.arena_top + L.staged);
                L.staged += j.acc.size();
            }
            FwSeg sg{};
            sg.X = j.X;
            sg.Y = j.Y;
            sg.acc_off = j.acc_dev_off;
            sg.acc_len = (int32_t)j.acc.size();
            sg.pad = j.rec = (int32_t)pool.nzrecs.size();  // index of the job's record in this launch
            fw_pool_cut(j.next, j.next + fw_pool_window(j.next, j.width, j.N), L.seglen, [&](uint64_t start, uint64_t end) {
                sg.start = start;
                sg.end = end;
                L.segs[si] = sg;
                pool.seg_job[si] = (int64_t)ji;
                ++si;
            });
            if (!L.nzs && !L.stream) continue;
            FwNzJob r{};  // fz_nz: sub-matrix of the job; recursive_pcor = 0: job-local correlation matrix
            r.X = j.X;
            r.Y = j.Y;
            r.acc_off = j.acc_dev_off;
            r.acc_len = (int32_t)j.acc.size();
            r.m = r.acc_len + 2;
            if (L.stream) {
                // the matrix of a job stays in the arena while the job lives: a job that takes several windows (pool rounds) has it
                // computed once (whole cfg3: fzs_gram_kernel was 30 % of the kernel time with one computation per round)
                if (j.gram_off < 0 || j.gram_epoch != pool.gram_epoch) {
                    j.gram_off = (int64_t)pool.gram_top;
                    j.gram_epoch = pool.gram_epoch;
                    pool.gram_top += (size_t)r.m * r.m;
                    r.nR = 1;  // to be computed in this launch
                    count_gram_job(c, r);
                }
                r.cor_off = (long long)j.gram_off;
                L.arena_floats = pool.gram_top;
            } else {
                r.cor_off = (long long)L.arena_floats;
                L.arena_floats += (size_t)r.m * r.m;
            }
            pool.nzrecs.push_back(r);
        }
        if (split && pass == 0) L.ns_tab = si;
    }
}

// recursive_pcor = 0: the job-matrix arena has to grow and loses its contents: every matrix of this launch is computed again at fresh
// offsets, dealt in pool.live order (the jobs that sit this round out are caught by the epoch)
static void pool_gram_regrow(fw_ctx *c, FwPool &pool, PoolLaunch &L)
{
    if (!L.stream || pool.gram_top * sizeof(double) <= c->d_arena.cap) return;
    pool.gram_epoch = ++c->gram_epoch;
    pool.gram_top = 0;
    for (size_t ji = 0; ji < pool.live.size(); ++ji) {
        FwPoolJob &j = pool.live[ji];
        if (!j.launched) continue;
        FwNzJob &r = pool.nzrecs[(size_t)j.rec];
        j.gram_off = (int64_t)pool.gram_top;
        j.gram_epoch = pool.gram_epoch;
        r.cor_off = (long long)j.gram_off;
        if (r.nR == 0) count_gram_job(c, r);  // a cached matrix that is computed again: counted like the ones pool_build_records scheduled
        r.nR = 1;
        pool.gram_top += (size_t)r.m * r.m;
    }
    L.arena_floats = pool.gram_top;
}

// the segment back-end of the context's kind and mode
static int pool_dispatch(fw_ctx *c, FwPool &pool, FwPoolBuf &pb, const PoolLaunch &L)
{
    const FwSeg *dsegs = (const FwSeg *)pb.d_in.ptr;
    const int32_t *dacc = (const int32_t *)pb.d_acc.ptr;
    const int64_t ns = (int64_t)L.ns, njobs = (int64_t)pool.nzrecs.size();
    if (L.nzs) {
        const bool f64 = !c->P.recursive_pcor;  // fz_nz without a matrix: Float64 view correlations, conditioned as StatsBase.partialcor does
        if (int rc = fwi_fznz_submatrices(c, njobs, pool.nzrecs.data(), L.arena_floats, dacc, pb.launch_stream, f64)) return rc;
        if (!f64) return fwi_fznz_segments(c, ns, (int64_t)L.ns_tab, dsegs, dacc, L.dout, pb);
        int m_max = 2;
        for (const FwNzJob &r : pool.nzrecs) m_max = std::max(m_max, (int)r.m);
        return fwi_fzs_segments_nz(c, ns, dsegs, dacc, L.dout, pb, m_max);
    }
    if (L.stream) {
        if (int rc = fwi_fzs_segments(c, ns, dsegs, dacc, L.dout, pb, pool.nzrecs.data(), njobs, L.arena_floats)) return rc;
        if (L.arena_floats * sizeof(double) > ((size_t)8 << 30))
            pool.gram_epoch = 0;  // fwi_fzs_segments streamed this launch instead (matrices beyond its arena limit): nothing was cached
        return FW_OK;
    }
    return c->f64 ? fwi_fz64_segments(c, ns, dsegs, dacc, L.dout, pb)
           : L.fz ? fwi_fz_segments(c, ns, (int64_t)L.ns_tab, dsegs, dacc, L.dout, pb)
                  : fwi_mi_segments(c, ns, dsegs, dacc, L.dout, pb);
}

// on the pool's stream: the launch's records and new accepted lists up, the kernels, the results back (unless they were written
// straight into pinned memory), the event fwi_pool_collect waits for
static int pool_enqueue(fw_ctx *c, FwPool &pool, FwPoolBuf &pb, const PoolLaunch &L)
{
    FW_HIP(c, hipMemcpyAsync(pb.d_in.ptr, pb.h_in.ptr, L.ns * sizeof(FwSeg), hipMemcpyHostToDevice, pb.launch_stream));
    if (L.staged)
        FW_HIP(c, hipMemcpyAsync((int32_t *)pb.d_acc.ptr + pool.arena_top, L.hacc, L.staged * sizeof(int32_t), hipMemcpyHostToDevice,
                                 pb.launch_stream));
    pool.arena_top += L.staged;
    if (int rc = pool_dispatch(c, pool, pb, L)) return rc;
    if ((void *)L.dout != pb.h_out.ptr)
        FW_HIP(c, hipMemcpyAsync(pb.h_out.ptr, pb.d_out.ptr, L.ns * sizeof(FwSegOut), hipMemcpyDeviceToHost, pb.launch_stream));
    FW_HIP(c, hipEventRecord(pb.evd, pb.launch_stream));
    return FW_OK;
}

int fwi_pool_launch(fw_ctx *c, FwPool &pool)
{
    pool.ns = 0;
    pool.inflight = false;
    pool_drop_stale(c, pool);
    if (pool.live.empty()) return FW_OK;
    if (pool_no_power(c)) {  // no device work: fwi_pool_collect fills the results
        pool.inflight = true;
        return FW_OK;
    }
    const double tb0 = fwi_now_s();
    FwPoolBuf &pb = c->pb[pool.buf];
    PoolLaunch L;
    pool_plan(c, pool, L);
    if (L.n_launch == 0) return FW_OK;  // everything is on hold: nothing to do this round
    if (int rc = pool_acc_arena(c, pool, pb, L)) return rc;
    if (int rc = pool_reserve_staging(c, pb, L)) return rc;
    pool_build_records(c, pool, L);
    pool_gram_regrow(c, pool, L);
    const double tb1 = fwi_now_s();
    c->cnt.t_host_build_s += tb1 - tb0;
    if (int rc = pool_enqueue(c, pool, pb, L)) return rc;
    pool.ns = L.ns;
    pool.inflight = true;
    pool.t_launch = fwi_now_s();
    c->cnt.t_host_launch_s += pool.t_launch - tb1;
    return FW_OK;
}

// ---- collect -----------------------------------------------------------------------------------------
// FW_TRACE_ROUNDS=<file>: one line per pool round (profiling aid; see profiles/README.md)
static void trace_round(const FwPool &pool, const FwSegOut *so, double kernel_us, double t_wait0, double t_wait1)
{
    static FILE *tf = [] {
        const char *e = fw_knob_str(knob::FW_TRACE_ROUNDS);
        return e ? fopen(e, "w") : (FILE *)nullptr;
    }();
    static double t_prev = 0.0;
    if (tf) {
        unsigned long long ev_sum = 0;
        for (size_t q = 0; q < pool.ns; ++q) ev_sum += so[q].evaluated;
        fprintf(tf, "%zu %zu %.1f %.1f %.1f %llu\n", pool.live.size(), pool.ns, kernel_us, 1e6 * (t_wait1 - t_wait0),
                t_prev > 0.0 ? 1e6 * (t_wait1 - t_prev) : 0.0, ev_sum);
        fflush(tf);
    }
    t_prev = t_wait1;
}

// FW_TRACE_JOBS=<file>: |accepted|, evaluated tests, reference-order tests, status per finished job
static void trace_job(const FwPoolJob &j)
{
    static FILE *jf = [] {
        const char *e = fw_knob_str(knob::FW_TRACE_JOBS);
        return e ? fopen(e, "w") : (FILE *)nullptr;
    }();
    if (jf) fprintf(jf, "%zu %lld %lld %d\n", j.acc.size(), (long long)j.out.evaluated, (long long)j.out.num_tests, j.out.status);
}

// FW_WINDOW_GROWTH is a tuning knob for profiling runs
static uint64_t pool_growth(size_t n_live, uint64_t launched_ranks)
{
    static const uint64_t forced = [] {
        const long v = (long)fw_knob_u64(knob::FW_WINDOW_GROWTH, 0ull);
        return (v >= 2 && v <= 64) ? (uint64_t)v : 0ull;
    }();
    static const uint64_t small = fw_small_launch();
    return fw_pool_growth(n_live, launched_ranks, forced, small);
}

// waits for the launch; returns the time of its kernels and when the wait began and ended
static int pool_wait(fw_ctx *c, FwPoolBuf &pb, float *kernel_ms, double *t0, double *t1)
{
    *t0 = fwi_now_s();
    FW_HIP(c, hipEventSynchronize(pb.evd));
    *t1 = fwi_now_s();
    c->cnt.t_host_wait_s += *t1 - *t0;
    FW_HIP(c, hipEventElapsedTime(kernel_ms, pb.ev0, pb.ev1));
    c->cnt.t_dev_subsets_s += 1e-3 * (double)*kernel_ms;
    c->cnt.kernel_launches += 1;
    c->cnt.subsets_launches += 1;
    return FW_OK;
}

// past the window, wider; finished jobs leave the pool in pool.live order
static void pool_advance(fw_ctx *c, FwPool &pool, std::vector<FwPoolJob> &finished)
{
    const uint64_t growth = pool_growth(pool.live.size(), pool.launched_ranks);
    size_t w = 0;
    for (size_t ji = 0; ji < pool.live.size(); ++ji) {
        FwPoolJob &j = pool.live[ji];
        if (!j.done && j.launched) fw_pool_advance(j, growth);
        if (j.done) {
            finish_job(c, j, pool.want_zs);
            trace_job(j);
            finished.push_back(std::move(j));
        } else {
            if (w != ji) pool.live[w] = std::move(j);
            ++w;
        }
    }
    pool.live.resize(w);
}

int fwi_pool_collect(fw_ctx *c, FwPool &pool, std::vector<FwPoolJob> &finished)
{
    if (!pool.inflight) return FW_OK;
    pool.inflight = false;
    if (pool_no_power(c)) {  // no launch was made: every live job returns the first test
        for (FwPoolJob &j : pool.live) {
            no_power_result(c, j.acc.data(), (int)j.acc.size(), j.out);
            j.done = true;
            finished.push_back(std::move(j));
        }
        pool.live.clear();
        return FW_OK;
    }
    FwPoolBuf &pb = c->pb[pool.buf];
    const FwSegOut *so = (const FwSegOut *)pb.h_out.ptr;
    float kernel_ms = 0.0f;
    double t_wait0 = 0.0, t_wait1 = 0.0;
    if (int rc = pool_wait(c, pb, &kernel_ms, &t_wait0, &t_wait1)) return rc;
    trace_round(pool, so, 1e3 * (double)kernel_ms, t_wait0, t_wait1);
    // in-order merge (segments of a job are contiguous and in rank order)
    for (size_t s = 0; s < pool.ns; ++s) fw_pool_merge(pool.live[(size_t)pool.seg_job[s]], so[s]);
    pool_advance(c, pool, finished);
    c->cnt.t_host_merge_s += fwi_now_s() - t_wait1;
    return FW_OK;
}

int fwi_pool_round(fw_ctx *c, FwPool &pool, std::vector<FwPoolJob> &finished)
{
    int rc = fwi_pool_launch(c, pool);
    if (rc) return rc;
    return fwi_pool_collect(c, pool, finished);
}

int fwi_subsets_dispatch(fw_ctx *c, int64_t m, const FwJob *jobs, const int32_t *acc, int64_t acc_total, FwJobOut *out)
{
    (void)acc_total;
    FwPool pool;
    pool.want_zs = true;
    for (int64_t i = 0; i < m; ++i) fwi_pool_add(c, pool, jobs[i].X, jobs[i].Y, acc + jobs[i].acc_off, jobs[i].acc_len, i);
    std::vector<FwPoolJob> fin;
    while (!pool.live.empty()) {
        int rc = fwi_pool_round(c, pool, fin);
        if (rc) return rc;
    }
    for (FwPoolJob &j : fin) out[j.tag] = j.out;
    return FW_OK;
}
