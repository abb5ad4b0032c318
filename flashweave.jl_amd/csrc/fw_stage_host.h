// The capacity policy of the level-0 drivers (fw_fz.hip, fw_fz64.hip, fw_mi.hip): plain C++17, no HIP and no fw_ctx, so that
// tests/native/stage_check.cpp can compile it with g++ alone (tests/test_stage_host_cpu.py).  fwi_l0_attempts (fw_internal.h) binds it
// to a context.
//
// A level-0 kernel appends its significant pairs to a buffer of `cap` entries and counts every pair it wanted to append.  The buffer
// is sized before the count is known: for min(pairs, limit) entries, or for the largest count an earlier call of the context saw
// (the hint: a repeated call does not overflow, and run the kernel, again).  A count beyond the capacity means one more attempt with
// exactly that count; a second overflow is an error (the data did not change in between).
#pragma once
#include <algorithm>
#include <string>

#include "../../include/flashweave_amd.h"

// Capacity of the first attempt: never 0, never below the hint.
inline unsigned long long fw_l0_first_cap(long long pairs, long long limit, unsigned long long hint)
{
    const unsigned long long cap = (unsigned long long)std::max<long long>(std::min(pairs, limit), 1);
    return std::max(cap, hint);
}

// What one attempt counted.  `first` is the count of its first (or only) stage and raises the hint; a driver of two stages (fz: screen,
// then the exact test of the screened pairs into a buffer of the same capacity) runs the second only when the first fitted and
// reports its count in `second`: beyond the capacity it asks for another attempt as well.
struct FwL0Counts {
    unsigned long long first = 0, second = 0;
};

// At most two attempts of run(cap, counts) -> FW_OK or the error that ends the call.  Returns FW_OK once every count fitted its
// capacity; FW_ERR_DEVICE with "<what> overflow twice" in `overflow` (left empty otherwise) after the second one that did not.
template <class Run>
inline int fw_l0_attempts(unsigned long long cap, unsigned long long &hint, const char *what, std::string &overflow, Run &&run)
{
    for (int attempt = 0; attempt < 2; ++attempt) {
        FwL0Counts n;
        if (const int rc = run(cap, n)) return rc;
        hint = std::max(hint, n.first);
        const unsigned long long need = std::max(n.first, n.second);
        if (need <= cap) return FW_OK;
        cap = need;
    }
    overflow = std::string(what) + " overflow twice";
    return FW_ERR_DEVICE;
}
