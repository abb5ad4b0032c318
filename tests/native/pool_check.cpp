// Host-side driver of csrc/fw_pool_host.h for tests/test_pool_host_cpu.py: no HIP, no library.  Reads whitespace-separated tokens from
// stdin (doubles as the 16 hex digits of their bits), first the mode:
//   enum    n then n x (a max_k max_tests)                          -> n lines: N
//   plan    fz seg_target forced small_launch w0_big max_k max_tests njobs a[njobs]
//           every job runs to its last rank          -> per launch "seglen nseg nwin" and nwin x "job lo hi" on one line
//   cut     lo hi seglen                                            -> "start end" per segment
//   merge   N next width then commands: seg <FwSegOut: stop_rank|none stop_stat stop_pval best_rank best_stat best_pval stop_df
//           stop_power best_df evaluated> | adv growth              -> the job's state, see put_state
//   unrank  a max_k n then n ranks                                  -> per rank "s pos..."
//   binom   fw_pool_binom against a long-double restatement with the same bounds: t = 0..7, m = 0..65 536 and 4 096 values of m on either
//           side of the first saturating m below 2^31                -> per t "t first_saturating_m|-1 mismatches"
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../flashweave.jl_amd/csrc/fw_pool_host.h"

static long long rd()
{
    long long v;
    if (!(std::cin >> v)) throw std::runtime_error("short input");
    return v;
}
static uint64_t rd_u64()
{
    std::string s;
    if (!(std::cin >> s)) throw std::runtime_error("short input");
    return s == "none" ? FW_RANK_NONE : strtoull(s.c_str(), nullptr, 10);
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
static uint64_t bits(double d)
{
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}

static int mode_enum()
{
    const int n = (int)rd();
    for (int i = 0; i < n; ++i) {
        const int a = (int)rd(), max_k = (int)rd();
        const int64_t max_tests = rd();
        printf("%" PRIu64 "\n", fw_pool_enum_size(a, max_k, max_tests));
    }
    return 0;
}

static int mode_plan()
{
    const bool fz = rd() != 0;
    const uint64_t seg_target = (uint64_t)rd(), forced = (uint64_t)rd(), small_launch = (uint64_t)rd(), w0_big = (uint64_t)rd();
    const int max_k = (int)rd();
    const int64_t max_tests = rd();
    std::vector<FwJobRun> jobs((size_t)rd());
    for (FwJobRun &j : jobs) {
        const int a = (int)rd();
        j.N = fw_pool_enum_size(a, max_k, max_tests);
        j.width = fw_pool_first_window(fz, a, w0_big);
    }
    for (;;) {
        uint64_t total = 0;
        size_t n_live = 0;
        for (const FwJobRun &j : jobs)
            if (!j.done) total += fw_pool_window(j.next, j.width, j.N), ++n_live;
        if (n_live == 0) return 0;
        const uint64_t seglen = fw_pool_seglen(total, fz, seg_target);
        uint64_t ns = 0;
        for (const FwJobRun &j : jobs)
            if (!j.done) ns += fw_pool_nsegs(fw_pool_window(j.next, j.width, j.N), seglen);
        printf("%" PRIu64 " %" PRIu64 " %zu", seglen, ns, n_live);
        const uint64_t growth = fw_pool_growth(n_live, total, forced, small_launch);
        for (size_t i = 0; i < jobs.size(); ++i) {
            FwJobRun &j = jobs[i];
            if (j.done) continue;
            printf(" %zu %" PRIu64 " %" PRIu64, i, j.next, j.next + fw_pool_window(j.next, j.width, j.N));
            fw_pool_advance(j, growth);
        }
        printf("\n");
    }
}

static int mode_cut()
{
    const uint64_t lo = rd_u64(), hi = rd_u64(), seglen = rd_u64();
    fw_pool_cut(lo, hi, seglen, [](uint64_t s, uint64_t e) { printf("%" PRIu64 " %" PRIu64 "\n", s, e); });
    return 0;
}

// "done no_zs next width best_rank best_df best_p best_stat | stat pval num_tests evaluated df suff_power status"
static void put_state(const FwJobRun &j)
{
    printf("%d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %d %016" PRIx64 " %016" PRIx64 " | %016" PRIx64 " %016" PRIx64 " %lld %lld %d %d %d\n", (int)j.done,
           (int)j.no_zs, j.next, j.width, j.best_rank, j.best_df, bits(j.best_p), bits(j.best_stat), bits(j.out.stat), bits(j.out.pval),
           (long long)j.out.num_tests, (long long)j.out.evaluated, j.out.df, j.out.suff_power, j.out.status);
}

static int mode_merge()
{
    FwJobRun j;
    j.N = rd_u64(), j.next = rd_u64(), j.width = rd_u64();
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "seg") {
            FwSegOut o{};
            o.stop_rank = rd_u64(), o.stop_stat = rd_bits(), o.stop_pval = rd_bits();
            o.best_rank = rd_u64(), o.best_stat = rd_bits(), o.best_pval = rd_bits();
            o.stop_df = (int32_t)rd(), o.stop_power = (int32_t)rd(), o.best_df = (int32_t)rd(), o.evaluated = rd_u64();
            fw_pool_merge(j, o);
        } else if (cmd == "adv") {
            const uint64_t growth = rd_u64();
            if (!j.done) fw_pool_advance(j, growth);  // (as the pool: a stopped job leaves, it does not advance)
        } else {
            return 2;
        }
    }
    put_state(j);
    return 0;
}

static int mode_unrank()
{
    const int a = (int)rd(), max_k = (int)rd();
    const int n = (int)rd();
    for (int i = 0; i < n; ++i) {
        int s = 0, pos[FW_MAX_K] = {0};
        fw_pool_unrank(rd_u64(), a, max_k, &s, pos);
        printf("%d", s);
        for (int q = 0; q < s; ++q) printf(" %d", pos[q]);
        printf("\n");
    }
    return 0;
}

// the reference form: 80-bit estimate of C(m, t) against 3.6e18 up to t = 5 and 2.0e18 for t = 6, 7, then the exact running product
static uint64_t binom_long_double(int64_t m, int t)
{
    if (t < 0 || m < t) return 0;
    long double r = 1.0L;
    for (int i = 1; i <= t; ++i) r = r * (long double)(m - t + i) / (long double)i;
    if (r > (t > 5 ? 2.0e18L : 3.6e18L)) return 1ull << 62;
    uint64_t v = 1;
    for (int i = 1; i <= t; ++i) v = v * (uint64_t)(m - t + i) / (uint64_t)i;
    return v;
}

static int mode_binom()
{
    const uint64_t SAT = 1ull << 62;
    for (int t = 0; t <= 7; ++t) {
        long long bad = 0;
        for (int64_t m = 0; m <= 65536; ++m) bad += binom_long_double(m, t) != fw_pool_binom(m, t);
        int64_t lo = 0, hi = (1ll << 31) - 1;
        if (binom_long_double(hi, t) != SAT) {
            printf("%d -1 %lld\n", t, bad);
            continue;
        }
        while (lo < hi) {  // (monotone in m)
            const int64_t mid = (lo + hi) / 2;
            if (binom_long_double(mid, t) == SAT)
                hi = mid;
            else
                lo = mid + 1;
        }
        for (int64_t m = lo - 4096; m < lo + 4096; ++m) bad += binom_long_double(m, t) != fw_pool_binom(m, t);
        printf("%d %lld %lld\n", t, (long long)lo, bad);
    }
    return 0;
}

int main()
{
    std::ios::sync_with_stdio(false);
    std::string mode;
    std::cin >> mode;
    try {
        if (mode == "enum") return mode_enum();
        if (mode == "plan") return mode_plan();
        if (mode == "cut") return mode_cut();
        if (mode == "merge") return mode_merge();
        if (mode == "unrank") return mode_unrank();
        if (mode == "binom") return mode_binom();
    } catch (const std::exception &e) {
        fprintf(stderr, "pool_check: %s\n", e.what());
        return 1;
    }
    return 2;
}
