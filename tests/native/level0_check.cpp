// Host-side driver of csrc/fw_level0_host.h for tests/test_level0_host_cpu.py: no HIP, no library.  Reads whitespace-separated tokens from
// stdin (doubles as the 16 hex digits of their bits), first the mode:
//   bh     k m p[k]                                        -> the k adjusted p-values
//   csr    p k alpha pi[k] pj[k] stat[k] adj_p[k]          -> four lines: off idx stat p
//   split  world npairs ntot then ntot x (i j stat p)      -> "nrec m k", then four lines: pi pj stat pval
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>

#include "../../flashweave.jl_amd/csrc/fw_level0_host.h"

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

static int mode_bh()
{
    const size_t k = (size_t)rd();
    const int64_t m = rd();
    std::vector<double> p(k);
    for (auto &x : p) x = rd_bits();
    fw_bh_adjust(p, m);
    put_bits(p);
    return 0;
}

static int mode_csr()
{
    const int p = (int)rd();
    const size_t k = (size_t)rd();
    const double alpha = rd_bits();
    std::vector<int32_t> pi(k), pj(k);
    std::vector<double> stat(k), adj(k);
    for (auto &x : pi) x = (int32_t)rd();
    for (auto &x : pj) x = (int32_t)rd();
    for (auto &x : stat) x = rd_bits();
    for (auto &x : adj) x = rd_bits();
    std::vector<int64_t> off{7, 7};  // stale contents: the call replaces them
    std::vector<int32_t> idx{7};
    std::vector<double> s{7.0}, q{7.0};
    fw_nb_csr(p, pi, pj, stat, adj, alpha, off, idx, s, q);
    put(off), put(idx), put_bits(s), put_bits(q);
    return 0;
}

static int mode_split()
{
    const int world = (int)rd();
    const int64_t npairs = rd(), ntot = rd();
    std::vector<int32_t> ai((size_t)ntot), aj((size_t)ntot);
    std::vector<double> as((size_t)ntot), ap((size_t)ntot);
    for (int64_t t = 0; t < ntot; ++t) ai[t] = (int32_t)rd(), aj[t] = (int32_t)rd(), as[t] = rd_bits(), ap[t] = rd_bits();
    std::vector<int32_t> pi, pj;
    std::vector<double> stat, pval;
    int64_t m = 0;
    const int nrec = fw_l0_split_gathered(ntot, ai.data(), aj.data(), as.data(), ap.data(), world, npairs, pi, pj, stat, pval, &m);
    printf("%d %lld %zu\n", nrec, (long long)m, pi.size());
    put(pi), put(pj), put_bits(stat), put_bits(pval);
    return 0;
}

int main()
{
    std::ios::sync_with_stdio(false);
    std::string mode;
    std::cin >> mode;
    try {
        if (mode == "bh") return mode_bh();
        if (mode == "csr") return mode_csr();
        if (mode == "split") return mode_split();
    } catch (const std::exception &e) {
        fprintf(stderr, "level0_check: %s\n", e.what());
        return 1;
    }
    return 2;
}
