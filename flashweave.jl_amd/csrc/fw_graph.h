// The host-only part of fw_learn_network (fw_hiton.cpp): plain C++17 over vectors, no HIP and no fw_ctx, so that
// tests/native/graph_check.cpp can compile it with g++ alone (tests/test_graph_cpu.py).
//   target order, rounds, deal to ranks      learning.jl:97-98, interleaved.jl:62,76-86
//   running feed-forward graph               interleaved.jl:136-140
//   make_weights / make_symmetric_graph      misc.jl:137-159, 201-272
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <functional>
#include <mutex>
#include <numeric>
#include <thread>
#include <vector>

inline double fwi_now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// Directed entries (target, neighbour, statistic, p) in arrival order: a target's entries arrive together, in PC insertion order.
// One flat list (vectors of vectors cost 120 000 small allocations per cfg4 pass).
struct FwDirected {
    std::vector<int32_t> t, u;
    std::vector<double> s, p;
    size_t size() const { return t.size(); }
    void reserve(size_t n) { t.reserve(n), u.reserve(n), s.reserve(n), p.reserve(n); }
    void resize(size_t n) { t.resize(n), u.resize(n), s.resize(n), p.resize(n); }
    void push(int32_t T, int32_t U, double S, double P) { t.push_back(T), u.push_back(U), s.push_back(S), p.push_back(P); }
    void append(const int32_t *T, const int32_t *U, const double *S, const double *P, size_t n)
    {
        t.insert(t.end(), T, T + n), u.insert(u.end(), U, U + n), s.insert(s.end(), S, S + n), p.insert(p.end(), P, P + n);
    }
};

// The level-0 neighbour lists (CSR over variables, ascending ids inside a list) as the passes read them.
struct FwLevel0 {
    int p = 0;
    const int64_t *off = nullptr;
    const int32_t *idx = nullptr;
    const double *stat = nullptr, *pval = nullptr;
    int64_t deg(int32_t T) const { return off[T + 1] - off[T]; }
    // position of v in T's list (an index into idx / stat / pval), -1 if v is not a neighbour of T
    int64_t find(int32_t T, int32_t v) const
    {
        const int32_t *b = idx + off[T], *e = idx + off[T + 1];
        const int32_t *it = std::lower_bound(b, e, v);
        return it != e && *it == v ? off[T] + (it - b) : -1;
    }
};

// learning.jl:97-98: ascending univariate degree, stable
inline std::vector<int32_t> fw_target_order(const FwLevel0 &l0)
{
    std::vector<int32_t> order((size_t)l0.p);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return l0.deg(a) < l0.deg(b); });
    return order;
}

// End of the round that starts at target r0 of nt (round_size <= 0: one round).
// R = 1 is the reference's single_il master: job_q_buff_size = 1, so the first TWO targets of the schedule are enqueued up front with
// an empty whitelist (interleaved.jl:62,76-86); from the third target on a job sees neighbors(graph, T).  The first round therefore
// holds two targets.
inline int fw_round_end(int r0, int round_size, int nt)
{
    const int R = round_size <= 0 ? nt : round_size;
    return (int)std::min<int64_t>(nt, (int64_t)r0 + ((R == 1 && r0 == 0) ? 2 : R));
}

// The rank that runs each target of the round order[r0 .. r1).  The targets of a round are independent of each other (whitelists only
// change between rounds), so any deal gives the same network; what matters is the balance.  r02 dealt them round-robin in schedule
// order, and at cfg3 / 8 ranks the heaviest rank carried 1.86e9 of the round's tests against a mean of 1.49e9.  Now:
// longest-processing-time-first on an estimate of a target's work -- the number of conditioning subsets its candidate list can span,
// C(deg, <= max_k) ~ deg^max_k (+ a constant for the chain of jobs every target pays) -- heaviest first, each to the least loaded
// rank, ties to the lower rank.  Every rank computes the same deal from the replicated level-0 lists.
inline std::vector<int32_t> fw_deal_round(const FwLevel0 &l0, const int32_t *order, int r0, int r1, int world, int max_k)
{
    std::vector<int32_t> owner((size_t)(r1 - r0), 0);
    if (world <= 1) return owner;
    // the schedule is sorted by ascending degree, and the estimate is monotone in the degree: heaviest first = the round's targets in
    // REVERSE schedule order (no sort; r03's first version sorted with pow() in the comparator: 15 ms per cfg4 round on every rank)
    const int kk = std::min(std::max(max_k, 1), 3);
    std::vector<double> load((size_t)world, 0.0);
    for (int32_t j = r1 - r0 - 1; j >= 0; --j) {
        const double d = (double)l0.deg(order[r0 + j]);
        const double est = (kk == 1 ? d : kk == 2 ? d * d : d * d * d) + 64.0;
        int best = 0;
        for (int w = 1; w < world; ++w)
            if (load[w] < load[best]) best = w;
        owner[j] = best;
        load[best] += est;
    }
    return owner;
}

// The running graph of the feed-forward schedule: a target's whitelist is its sorted neighbour list, only modified between rounds.
struct FwRunningGraph {
    std::vector<std::vector<int32_t>> adj;
    std::vector<uint8_t> is_dirty;
    std::vector<int32_t> dirty;
    explicit FwRunningGraph(int p) : adj((size_t)p), is_dirty((size_t)p, 0) {}
    // interleaved.jl:136-140 add_edge! (idempotent): both directions appended, the touched lists sorted and de-duplicated once per
    // round (sorted inserts one entry at a time were 15 ms of a 170 ms cfg4 pass)
    void add(const int32_t *t, const int32_t *u, int64_t n)
    {
        for (int64_t i = 0; i < n; ++i) {
            adj[t[i]].push_back(u[i]);
            adj[u[i]].push_back(t[i]);
            if (!is_dirty[t[i]]) is_dirty[t[i]] = 1, dirty.push_back(t[i]);
            if (!is_dirty[u[i]]) is_dirty[u[i]] = 1, dirty.push_back(u[i]);
        }
        for (int32_t v : dirty) {
            std::vector<int32_t> &l = adj[v];
            std::sort(l.begin(), l.end());
            l.erase(std::unique(l.begin(), l.end()), l.end());
            is_dirty[v] = 0;
        }
        dirty.clear();
    }
    const int32_t *whitelist(int32_t T, int *n) const
    {
        *n = (int)adj[T].size();
        return adj[T].empty() ? nullptr : adj[T].data();
    }
};

// Host threads of the graph passes, kept for the life of the context: starting fifteen threads per pass cost more than the passes' work
// at cfg3 (2.4 of 2.8 ms for 48 040 edges; r05).  run(fn, b): fn(w, b[w], b[w + 1]) for every block w, block 0 on the caller.
struct FwHostWorkers {
    typedef std::function<void(int, int, int)> Fn;
    std::vector<std::thread> th;
    std::mutex mu;
    std::condition_variable cv_go, cv_done;
    const Fn *fn = nullptr;
    const int *blk = nullptr;
    unsigned long long gen = 0;
    int pending = 0;
    bool quit = false, failed = false;
    explicit FwHostWorkers(int n)
    {
        for (int w = 1; w < n; ++w) th.emplace_back([this, w] { loop(w); });
    }
    int blocks() const { return (int)th.size() + 1; }
    void loop(int w)
    {
        unsigned long long seen = 0;
        for (;;) {
            const Fn *f;
            const int *b;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv_go.wait(lk, [&] { return quit || gen != seen; });
                if (quit) return;
                seen = gen;
                f = fn;
                b = blk;
            }
            bool ok = true;
            try {
                (*f)(w, b[w], b[w + 1]);
            } catch (...) {  // (std::bad_alloc of a block-local vector: an exception that leaves a thread is std::terminate)
                ok = false;
            }
            std::lock_guard<std::mutex> lk(mu);
            if (!ok) failed = true;
            if (--pending == 0) cv_done.notify_one();
        }
    }
    // false: a block threw (out of memory).  The workers hold pointers to the caller's function object and block list, so the call
    // never leaves -- normally or by an exception of block 0 -- before every worker has finished its block (r05 unwound past them).
    bool run(const Fn &f, const int *b)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            fn = &f;
            blk = b;
            pending = (int)th.size();
            failed = false;
            ++gen;
        }
        cv_go.notify_all();
        bool ok0 = true;
        try {
            f(0, b[0], b[1]);
        } catch (...) {
            ok0 = false;
        }
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return pending == 0; });
        return ok0 && !failed;
    }
    ~FwHostWorkers()
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            quit = true;
        }
        cv_go.notify_all();
        for (std::thread &t : th) t.join();
    }
};

// The network: directed CSR over targets (arrival order inside a target = PC insertion order) and the undirected edge list.
struct FwNetwork {
    std::vector<int64_t> pc_off;
    std::vector<int32_t> pc_idx;
    std::vector<double> pc_w, pc_p;
    std::vector<int32_t> e_src, e_dst;
    std::vector<double> e_w;
};

// The passes walk the directed CSR with data-dependent look-ups: contiguous blocks of variables on a few host threads, every block into
// its own vectors, concatenated in block order -- the same edge list as the sequential loop.  n == 1: the caller alone, no workers.
struct FwBlocks {
    int p, n;
    FwHostWorkers *workers;  // n > 1: n - 1 threads
    std::vector<int> cut;    // block w = variables [cut[w], cut[w + 1])
    bool ok = true;          // false: a block ran out of memory (no exception crosses the C ABI); later passes are skipped
    FwBlocks(int p_, int n_, FwHostWorkers *w) : p(p_), n(n_), workers(w), cut((size_t)n_ + 1, p_) { cut[0] = 0; }
    // block w starts where the entries before it reach w / n of the total
    void cut_by(const std::vector<int64_t> &off)
    {
        for (int w = 1; w < n; ++w) {
            const int64_t want = off[(size_t)p] * w / n;
            cut[w] = std::min(p, (int)(std::lower_bound(off.begin(), off.end(), want) - off.begin()));
        }
    }
    void run(const FwHostWorkers::Fn &fn)
    {
        if (!ok) return;
        if (n > 1) {
            ok = workers->run(fn, cut.data());
            return;
        }
        try {
            fn(0, 0, p);
        } catch (...) {
            ok = false;
        }
    }
};

// CSR over targets (stable).  The scatter: every block reads the whole arrival list and places the entries of its own targets, in
// arrival order (one thread: 1.2 ms of random writes for cfg4's 157 000 entries)
inline void fw_directed_csr(FwBlocks &B, const FwDirected &d, FwNetwork &g)
{
    const size_t ne = d.size();
    g.pc_off.assign((size_t)B.p + 1, 0);
    for (size_t i = 0; i < ne; ++i) g.pc_off[(size_t)d.t[i] + 1]++;
    for (int T = 0; T < B.p; ++T) g.pc_off[T + 1] += g.pc_off[T];
    g.pc_idx.resize(ne);
    g.pc_w.resize(ne);
    g.pc_p.resize(ne);
    B.cut_by(g.pc_off);
    B.run([&](int, int lo, int hi) {
        if (lo >= hi) return;
        std::vector<int64_t> fill(g.pc_off.begin() + lo, g.pc_off.begin() + hi);
        for (size_t i = 0; i < ne; ++i) {
            const int32_t T = d.t[i];
            if (T < lo || T >= hi) continue;
            const int64_t q = fill[(size_t)(T - lo)]++;
            g.pc_idx[q] = d.u[i];
            g.pc_w[q] = d.s[i];
            g.pc_p[q] = d.p[i];
        }
    });
}

// misc.jl:137-159 make_weights ("cond_stat"): discrete tests take the sign of the univariate statistic
inline void fw_make_weights(FwBlocks &B, const FwLevel0 &l0, FwNetwork &g)
{
    B.run([&](int, int lo, int hi) {
        for (int T = lo; T < hi; ++T)
            for (int64_t i = g.pc_off[T]; i < g.pc_off[T + 1]; ++i) {
                const int64_t q = l0.find(T, g.pc_idx[i]);
                const double us = q >= 0 ? l0.stat[q] : NAN;
                const double sg = std::isnan(us) ? NAN : (double)((us > 0) - (us < 0));
                g.pc_w[i] = sg * std::fabs(g.pc_w[i]);
            }
    });
}

// Incoming lists (b -> a for every a) with their weights, ascending in b: the transpose of the CSR by counting sort.  The edge pass
// then reads two contiguous ranges per variable; looking the reverse direction up in b's own list instead cost two or three cache
// lines from another core per entry (cfg4: 3.1-5.0 ms on 16 / 8 threads for 380 000 entries; r05).
struct FwIncoming {
    std::vector<int64_t> off;
    std::vector<int32_t> idx;
    std::vector<double> w;
};
inline FwIncoming fw_transpose(int p, const FwNetwork &g)
{
    const size_t ne = g.pc_idx.size();
    FwIncoming in{std::vector<int64_t>((size_t)p + 1, 0), std::vector<int32_t>(ne), std::vector<double>(ne)};
    for (size_t i = 0; i < ne; ++i) in.off[(size_t)g.pc_idx[i] + 1]++;
    for (int T = 0; T < p; ++T) in.off[T + 1] += in.off[T];
    std::vector<int64_t> fill(in.off.begin(), in.off.end() - 1);
    for (int T = 0; T < p; ++T)  // sources visited in ascending order -> every incoming list comes out sorted
        for (int64_t i = g.pc_off[T]; i < g.pc_off[T + 1]; ++i) {
            const int64_t q = fill[g.pc_idx[i]]++;
            in.idx[(size_t)q] = T;
            in.w[(size_t)q] = g.pc_w[i];
        }
    return in;
}

inline double fw_maxweight(double w1, double w2)
{  // misc.jl:201-218
    if (std::isnan(w1)) return w2;
    if (std::isnan(w2)) return w1;
    const double s1 = (w1 > 0) - (w1 < 0), s2 = (w2 > 0) - (w2 < 0);
    if (s1 * s2 < 0) return w1;  // "arbitrarily choosing one": the lower-index endpoint's direction
    return std::max(std::fabs(w1), std::fabs(w2)) * s1;
}

struct FwGraphTimes {  // what the FW_TRACE_HOST lines of the passes print (seconds)
    double csr = 0, signs = 0, transpose = 0, edges = 0;                                // the four passes (edges: concatenation included)
    double latest_start = 0, longest_block = 0, edges_return = 0, concatenation = 0;  // inside the edge pass
};

// misc.jl:230-272 make_symmetric_graph (OR rule, maxweight merge, NaN edges dropped).  Block w's edges in (a ascending; outgoing entries
// in PC order, then incoming-only entries ascending in b), blocks concatenated in order.
inline void fw_symmetric_graph(FwBlocks &B, const FwIncoming &in, FwNetwork &g, FwGraphTimes &tm)
{
    const double t_call = fwi_now_s();
    std::vector<std::vector<int32_t>> bs((size_t)B.n), bd((size_t)B.n);
    std::vector<std::vector<double>> bw((size_t)B.n);
    std::vector<double> w_t0((size_t)B.n, t_call), w_t1((size_t)B.n, t_call);
    B.run([&](int w, int lo, int hi) {
        w_t0[(size_t)w] = fwi_now_s();
        std::vector<int32_t> es, ed;  // block-local, handed over at the end: the headers of bs[w], bs[w + 1] share cache lines and every
        std::vector<double> ew;       // push_back writes one (150 ns per entry on 8 threads; r05)
        const size_t room = (size_t)(g.pc_off[hi] - g.pc_off[lo]);
        es.reserve(room);
        ed.reserve(room);
        ew.reserve(room);
        auto emit = [&](int32_t a, int32_t b, double ww) {
            if (std::isnan(ww)) return;
            es.push_back(a);
            ed.push_back(b);
            ew.push_back(ww);
        };
        std::vector<int32_t> out_of((size_t)B.p, -1);  // out_of[b] == a: the direction a -> b exists
        for (int a = lo; a < hi; ++a) {
            const int32_t *ib = in.idx.data() + in.off[a], *ie = in.idx.data() + in.off[a + 1];
            for (int64_t i = g.pc_off[a]; i < g.pc_off[a + 1]; ++i) {  // direction a -> b exists
                const int32_t b = g.pc_idx[i];
                out_of[(size_t)b] = a;
                if (b <= a) continue;
                const int32_t *it = std::lower_bound(ib, ie, b);
                emit(a, b, fw_maxweight(g.pc_w[i], (it != ie && *it == b) ? in.w[(size_t)(in.off[a] + (it - ib))] : NAN));
            }
            for (int64_t q = in.off[a]; q < in.off[a + 1]; ++q) {  // only b -> a exists
                const int32_t b = in.idx[(size_t)q];
                if (b > a && out_of[(size_t)b] != a) emit(a, b, fw_maxweight(in.w[(size_t)q], NAN));
            }
        }
        bs[(size_t)w] = std::move(es);
        bd[(size_t)w] = std::move(ed);
        bw[(size_t)w] = std::move(ew);
        w_t1[(size_t)w] = fwi_now_s();
    });
    const double t_ret = fwi_now_s();
    g.e_src.clear();
    g.e_dst.clear();
    g.e_w.clear();
    for (int w = 0; B.ok && w < B.n; ++w) {
        g.e_src.insert(g.e_src.end(), bs[(size_t)w].begin(), bs[(size_t)w].end());
        g.e_dst.insert(g.e_dst.end(), bd[(size_t)w].begin(), bd[(size_t)w].end());
        g.e_w.insert(g.e_w.end(), bw[(size_t)w].begin(), bw[(size_t)w].end());
        tm.latest_start = std::max(tm.latest_start, w_t0[(size_t)w] - t_call);
        tm.longest_block = std::max(tm.longest_block, w_t1[(size_t)w] - w_t0[(size_t)w]);
    }
    tm.edges_return = t_ret - t_call;
    tm.concatenation = fwi_now_s() - t_ret;
}

// Directed entries -> network: the four passes on `blocks` blocks (workers: blocks - 1 threads, may be null for one block).
// false: a block ran out of memory.
inline bool fw_graph_passes(const FwLevel0 &l0, const FwDirected &d, bool discrete, int blocks, FwHostWorkers *workers, FwNetwork &g,
                            FwGraphTimes &tm)
{
    FwBlocks B(l0.p, blocks, workers);
    const double t0 = fwi_now_s();
    fw_directed_csr(B, d, g);
    const double t1 = fwi_now_s();
    if (discrete) fw_make_weights(B, l0, g);
    const double t2 = fwi_now_s();
    const FwIncoming in = fw_transpose(l0.p, g);
    const double t3 = fwi_now_s();
    fw_symmetric_graph(B, in, g, tm);
    tm.csr = t1 - t0, tm.signs = t2 - t1, tm.transpose = t3 - t2, tm.edges = fwi_now_s() - t3;
    return B.ok;
}
