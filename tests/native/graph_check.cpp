// Host-side driver of csrc/fw_graph.h for tests/test_graph_cpu.py: no HIP, no library.  Reads whitespace-separated tokens from stdin
// (doubles as the 16 hex digits of their bits, so that NaN, -0.0 and every last bit survive the text), first the mode:
//   graph  p discrete | level-0 CSR: nnz off[p+1] idx[nnz] stat[nnz] | directed list: ne then ne x (t u s pval) | nb then nb x (blocks reps)
//          -> per (blocks, rep): "run blocks rep" and the seven arrays pc_off pc_idx pc_w pc_p e_src e_dst e_w, one per line
//   throw  n k    n blocks on one FwHostWorkers, block k throws -> "ret R ended E next N"
//   sched  p off[p+1] then commands: order | end r0 round_size nt | deal r0 r1 world max_k
//   running p then commands: add n, n x (t u) | lists
#include <atomic>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>

#include "../../flashweave.jl_amd/csrc/fw_graph.h"

static long long rd()
{
    long long v;
    if (!(std::cin >> v)) throw std::runtime_error("short input");
    return v;
}
static double rd_bits()
{
    std::string s;
    if (!(std::cin >> s)) throw std::runtime_error("short input");
    const uint64_t b = strtoull(s.c_str(), nullptr, 16);
    double d;
    memcpy(&d, &b, 8);
    return d;
}
template <class V> static void put(const V &v)
{
    for (auto x : v) printf("%lld ", (long long)x);
    printf("\n");
}
static void put_bits(const std::vector<double> &v)
{
    for (double d : v) {
        uint64_t b;
        memcpy(&b, &d, 8);
        printf("%016" PRIx64 " ", b);
    }
    printf("\n");
}

static int mode_graph()
{
    const int p = (int)rd(), discrete = (int)rd();
    const size_t nnz = (size_t)rd();
    std::vector<int64_t> off((size_t)p + 1);
    std::vector<int32_t> idx(nnz);
    std::vector<double> stat(nnz), pval(nnz, 0.0);
    for (auto &x : off) x = rd();
    for (auto &x : idx) x = (int32_t)rd();
    for (auto &x : stat) x = rd_bits();
    const FwLevel0 l0{p, off.data(), idx.data(), stat.data(), pval.data()};
    FwDirected d;
    const size_t ne = (size_t)rd();
    d.reserve(ne);
    for (size_t i = 0; i < ne; ++i) {
        const int32_t t = (int32_t)rd(), u = (int32_t)rd();
        const double s = rd_bits(), pv = rd_bits();
        d.push(t, u, s, pv);
    }
    const int nb = (int)rd();
    for (int q = 0; q < nb; ++q) {
        const int blocks = (int)rd(), reps = (int)rd();
        FwHostWorkers workers(blocks);  // one object for all repetitions (blocks = 1: no thread)
        for (int r = 0; r < reps; ++r) {
            FwNetwork g;
            FwGraphTimes tm;
            if (!fw_graph_passes(l0, d, discrete != 0, blocks, &workers, g, tm)) return 3;
            printf("run %d %d\n", blocks, r);
            put(g.pc_off), put(g.pc_idx), put_bits(g.pc_w), put_bits(g.pc_p), put(g.e_src), put(g.e_dst), put_bits(g.e_w);
        }
    }
    return 0;
}

// a block function that throws: run() must report it, and only after every other block has ended
static int mode_throw()
{
    const int n = (int)rd(), k = (int)rd();
    FwHostWorkers workers(n);
    std::vector<int> cut((size_t)n + 1);
    std::iota(cut.begin(), cut.end(), 0);
    std::atomic<int> ended{0};
    const FwHostWorkers::Fn bad = [&](int w, int lo, int hi) {
        if (lo != w || hi != w + 1) throw std::logic_error("block bounds");
        if (w == k) throw std::bad_alloc();
        std::this_thread::sleep_for(std::chrono::milliseconds(20 + 5 * w));
        ++ended;
    };
    const bool ret = workers.run(bad, cut.data());
    const int seen = ended.load();  // read right behind the call: nothing may still be running
    std::atomic<int> good_n{0};
    const FwHostWorkers::Fn good = [&](int, int, int) { ++good_n; };
    const bool next = workers.run(good, cut.data()) && workers.run(good, cut.data());
    printf("ret %d ended %d next %d good %d\n", (int)ret, seen, (int)next, good_n.load());
    return 0;
}

static int mode_sched()
{
    const int p = (int)rd();
    std::vector<int64_t> off((size_t)p + 1);
    for (auto &x : off) x = rd();
    const FwLevel0 l0{p, off.data(), nullptr, nullptr, nullptr};
    const std::vector<int32_t> order = fw_target_order(l0);
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "order") {
            put(order);
        } else if (cmd == "end") {
            const int r0 = (int)rd(), rs = (int)rd(), nt = (int)rd();
            printf("%d\n", fw_round_end(r0, rs, nt));
        } else if (cmd == "deal") {
            const int r0 = (int)rd(), r1 = (int)rd(), world = (int)rd(), max_k = (int)rd();
            put(fw_deal_round(l0, order.data(), r0, r1, world, max_k));
        } else {
            return 2;
        }
    }
    return 0;
}

static int mode_running()
{
    const int p = (int)rd();
    FwRunningGraph graph(p);
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "add") {
            const size_t n = (size_t)rd();
            std::vector<int32_t> t(n), u(n);
            for (size_t i = 0; i < n; ++i) t[i] = (int32_t)rd(), u[i] = (int32_t)rd();
            graph.add(t.data(), u.data(), (int64_t)n);
        } else if (cmd == "lists") {
            for (int v = 0; v < p; ++v) {
                int n = 0;
                const int32_t *wl = graph.whitelist(v, &n);
                if ((wl == nullptr) != (n == 0)) return 4;
                put(std::vector<int32_t>(wl, wl + n));
            }
        } else {
            return 2;
        }
    }
    return 0;
}

int main()
{
    std::ios::sync_with_stdio(false);
    std::string mode;
    std::cin >> mode;
    try {
        if (mode == "graph") return mode_graph();
        if (mode == "throw") return mode_throw();
        if (mode == "sched") return mode_sched();
        if (mode == "running") return mode_running();
    } catch (const std::exception &e) {
        fprintf(stderr, "graph_check: %s\n", e.what());
        return 1;
    }
    return 2;
}
