// Position arithmetic of the CSC-resident fz_nz layout (fw_set_data_csc_f32_resident), usable from host and
// device code: the kernels of fw_fz.hip and the native check tests/native/cscres_check.cpp compile the same functions.
//
//   plane[c][w]   bit i: sample 64 w + i of column c has a value != 0.0f                       (uint64, [p][W], W = ceil(n / 64))
//   base[c][w]    position in vals of the first entry of column c at or after row 64 w:        (uint32, [p][W])
//                 the column's start plus the popcount of its plane words before w
//   vals          the values != 0.0f of all columns, column after column, rows ascending       (float, [nnz'])
//
// A column's run in vals has exactly one entry per set plane bit, so the entry of (c, row) -- when its bit is set -- sits at
// base[c][row >> 6] + popcount(plane[c][row >> 6] & bits below (row & 63)).
#ifndef FW_CSCRES_H
#define FW_CSCRES_H
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FW_CSCRES_HD __host__ __device__ __forceinline__
#else
#define FW_CSCRES_HD inline
#endif

FW_CSCRES_HD int fw_cscres_popc(unsigned long long x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

// bits of a plane word below position `bit` (0 .. 63)
FW_CSCRES_HD unsigned long long fw_cscres_below(int bit) { return (1ull << bit) - 1ull; }

// position in vals of the entry at bit `bit` of a plane word `m` whose base is `base`; the bit must be set in m
FW_CSCRES_HD uint32_t fw_cscres_pos(unsigned long long m, uint32_t base, int bit)
{
    return base + (uint32_t)fw_cscres_popc(m & fw_cscres_below(bit));
}

// value of (column, row) from the column's plane words, its base words and vals: 0.0f where the bit is clear.  The load is
// unconditional (position 0 stands in for an absent entry; vals always holds at least one float) so that the loads of several
// columns of one row can be in flight together instead of each waiting behind its own branch.
FW_CSCRES_HD float fw_cscres_word_value(unsigned long long m, uint32_t base, const float *vals, int bit)
{
    const bool set = (m >> bit) & 1ull;
    const float v = vals[set ? fw_cscres_pos(m, base, bit) : 0u];
    return set ? v : 0.0f;
}

FW_CSCRES_HD float fw_cscres_value(const unsigned long long *plane_col, const uint32_t *base_col, const float *vals, int row)
{
    return fw_cscres_word_value(plane_col[row >> 6], base_col[row >> 6], vals, row & 63);
}

#endif
