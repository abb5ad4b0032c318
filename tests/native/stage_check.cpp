// Host-side driver of csrc/fw_stage_host.h for tests/test_stage_host_cpu.py: no HIP, no library.  Reads whitespace-separated tokens
// from stdin, first the mode:
//   cap       pairs limit hint                              -> the first capacity
//   attempts  cap hint what nscript then nscript x (first second)
//             every attempt consumes the next scripted pair of counts ("what" is one token, '~' for a blank)
//             -> "rc hint nattempts", the capacities the attempts were given, the overflow message (may be empty)
// A script that runs out ends the program with an error: the loop asked for more attempts than the caller allowed.
#include <cstdio>
#include <iostream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../flashweave.jl_amd/csrc/fw_stage_host.h"

static long long rd()
{
    long long v;
    if (!(std::cin >> v)) throw std::runtime_error("short input");
    return v;
}

static int mode_cap()
{
    const long long pairs = rd(), limit = rd();
    const unsigned long long hint = (unsigned long long)rd();
    printf("%llu\n", fw_l0_first_cap(pairs, limit, hint));
    return 0;
}

static int mode_attempts()
{
    unsigned long long cap = (unsigned long long)rd(), hint = (unsigned long long)rd();
    std::string what;
    if (!(std::cin >> what)) throw std::runtime_error("short input");
    for (char &c : what)
        if (c == '~') c = ' ';
    std::vector<FwL0Counts> script((size_t)rd());
    for (auto &n : script) n.first = (unsigned long long)rd(), n.second = (unsigned long long)rd();
    std::vector<unsigned long long> caps;
    std::string overflow;
    const int rc = fw_l0_attempts(cap, hint, what.c_str(), overflow, [&](unsigned long long c, FwL0Counts &n) -> int {
        if (caps.size() >= script.size()) throw std::runtime_error("more attempts than scripted");
        n = script[caps.size()];
        caps.push_back(c);
        return n.first == 99999 ? FW_ERR_NOMEM : FW_OK;  // (a scripted failure of the attempt itself)
    });
    printf("%d %llu %zu\n", rc, hint, caps.size());
    for (unsigned long long c : caps) printf("%llu ", c);
    printf("\n%s\n", overflow.c_str());
    return 0;
}

int main()
{
    std::ios::sync_with_stdio(false);
    std::string mode;
    std::cin >> mode;
    try {
        if (mode == "cap") return mode_cap();
        if (mode == "attempts") return mode_attempts();
    } catch (const std::exception &e) {
        fprintf(stderr, "stage_check: %s\n", e.what());
        return 1;
    }
    return 2;
}
