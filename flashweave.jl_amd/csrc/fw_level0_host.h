// The host-only part of level 0 (fw_core.cpp): plain C++17 over vectors, no HIP and no fw_ctx, so that
// tests/native/level0_check.cpp can compile it with g++ alone (tests/test_level0_host_cpu.py).
//   Benjamini-Hochberg on the significant pairs      statfuns.jl:326-350
//   neighbour lists (CSR, partners ascending)        tests.jl:372-388
//   split of an all-gathered record list             fw_level0_sharded
// The first two are the host restatement of fw_bh.hip that FW_HOST_BH=1 selects and tests/test_gpu_fz.py holds the device to, bit for bit.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

// BH adjustment of the p-values of the k significant pairs, in place, for m tests in all.  Ascending sort by p: LSD radix sort on the
// IEEE bit pattern (p >= 0 -> order preserving).  Ties need no stable order: the backward cumulative minimum gives every member of a
// tie group the same value.
inline void fw_bh_adjust(std::vector<double> &pval, int64_t m)
{
    const size_t k = pval.size();
    if (k == 0) return;
    std::vector<uint64_t> key(k), key2(k);
    std::vector<uint32_t> val(k), val2(k);
    for (size_t t = 0; t < k; ++t) {
        memcpy(&key[t], &pval[t], 8);
        val[t] = (uint32_t)t;
    }
    std::vector<uint32_t> hist(65536);
    for (int pass = 0; pass < 4; ++pass) {
        const int sh = 16 * pass;
        std::fill(hist.begin(), hist.end(), 0u);
        for (size_t t = 0; t < k; ++t) hist[(key[t] >> sh) & 0xFFFF]++;
        uint32_t run = 0;
        for (size_t d = 0; d < 65536; ++d) {
            const uint32_t h = hist[d];
            hist[d] = run;
            run += h;
        }
        for (size_t t = 0; t < k; ++t) {
            const uint32_t dst = hist[(key[t] >> sh) & 0xFFFF]++;
            key2[dst] = key[t];
            val2[dst] = val[t];
        }
        key.swap(key2);
        val.swap(val2);
    }
    const double md = (double)m;
    double next_adj = 0.0;
    for (size_t i = k; i-- > 0;) {
        double pv;
        memcpy(&pv, &key[i], 8);
        double adj = pv * md / (double)(i + 1);
        if (i == k - 1)
            adj = std::min(adj, 1.0);
        else
            adj = std::min(next_adj, adj);
        next_adj = adj;
        pval[val[i]] = adj;
    }
}

// Neighbour lists of p variables from the pairs (pi < pj) with adjusted p < alpha, partners ascending.  Two stable counting sorts give
// the (X ascending, Y ascending) pair order of the reference's condensed arrays, whatever order the pairs arrive in; appending in that
// order yields ascending partner lists for both endpoints.
inline void fw_nb_csr(int p, const std::vector<int32_t> &pi, const std::vector<int32_t> &pj, const std::vector<double> &stat,
                      const std::vector<double> &adj_p, double alpha, std::vector<int64_t> &nb_off, std::vector<int32_t> &nb_idx,
                      std::vector<double> &nb_stat, std::vector<double> &nb_p)
{
    const size_t k = pi.size();
    std::vector<uint32_t> keep;
    keep.reserve(k);
    for (size_t t = 0; t < k; ++t)
        if (adj_p[t] < alpha) keep.push_back((uint32_t)t);
    const size_t kk = keep.size();
    std::vector<uint32_t> byj(kk), byij(kk);
    {
        std::vector<uint32_t> cnt((size_t)p + 1, 0);
        for (uint32_t t : keep) cnt[pj[t] + 1]++;
        for (int v = 0; v < p; ++v) cnt[v + 1] += cnt[v];
        for (uint32_t t : keep) byj[cnt[pj[t]]++] = t;
        std::fill(cnt.begin(), cnt.end(), 0u);
        for (uint32_t t : byj) cnt[pi[t] + 1]++;
        for (int v = 0; v < p; ++v) cnt[v + 1] += cnt[v];
        for (uint32_t t : byj) byij[cnt[pi[t]]++] = t;
    }
    nb_off.assign((size_t)p + 1, 0);
    for (uint32_t t : byij) {
        nb_off[pi[t] + 1]++;
        nb_off[pj[t] + 1]++;
    }
    for (int v = 0; v < p; ++v) nb_off[v + 1] += nb_off[v];
    const int64_t tot = nb_off[p];
    nb_idx.assign((size_t)tot, 0);
    nb_stat.assign((size_t)tot, 0.0);
    nb_p.assign((size_t)tot, 0.0);
    std::vector<int64_t> fill(nb_off.begin(), nb_off.end() - 1);
    for (uint32_t t : byij) {
        const int X = pi[t], Y = pj[t];
        const int64_t a = fill[X]++, b = fill[Y]++;
        nb_idx[a] = Y;
        nb_stat[a] = stat[t];
        nb_p[a] = adj_p[t];
        nb_idx[b] = X;
        nb_stat[b] = stat[t];
        nb_p[b] = adj_p[t];
    }
}

// Sharded level 0 through a host all-gather: every rank appends one count record (i = -1, j = rank, stat = its number of reliable
// tests) to its significant pairs.  This splits the gathered list back into the pairs (in arrival order) and the merged count
//   m = sum_r m_r - (world - 1) * npairs      (every rank reports npairs minus ITS unreliable pairs).
// Returns the number of count records seen; anything but `world` is an error of the exchange (the outputs are then not to be used).
inline int fw_l0_split_gathered(int64_t ntot, const int32_t *ai, const int32_t *aj, const double *as, const double *ap, int world,
                                int64_t npairs, std::vector<int32_t> &pi, std::vector<int32_t> &pj, std::vector<double> &stat,
                                std::vector<double> &pval, int64_t *m)
{
    pi.clear(), pj.clear(), stat.clear(), pval.clear();
    pi.reserve((size_t)ntot), pj.reserve((size_t)ntot), stat.reserve((size_t)ntot), pval.reserve((size_t)ntot);
    int64_t msum = 0;
    int nrec = 0;
    for (int64_t t = 0; t < ntot; ++t) {
        if (ai[t] < 0) {
            msum += (int64_t)as[t];
            ++nrec;
            continue;
        }
        pi.push_back(ai[t]);
        pj.push_back(aj[t]);
        stat.push_back(as[t]);
        pval.push_back(ap[t]);
    }
    *m = msum - (int64_t)(world - 1) * npairs;
    return nrec;
}
