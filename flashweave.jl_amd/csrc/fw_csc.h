// Structure check of a CSC triple on the device, shared by the two entry points that take one from the caller and read it in
// kernels (fw_normalize_counts_csc in fw_norm.hip, fw_set_data_csc_f32 in fw_fz.hip): one wavefront per column, one pass.
// A column is good when colptr[j] <= colptr[j+1] lie in 0 .. nnz and its rows are 0 <= row < n, strictly ascending.  Nothing
// outside [0, nnz) is read, so a broken colptr cannot make the check itself fault.
#ifndef FW_CSC_H
#define FW_CSC_H
#include <cstdint>

#include <hip/hip_runtime.h>

enum {
    FW_CSC_BAD_COLPTR = 1,  // colptr[j] > colptr[j+1], or outside 0 .. nnz
    FW_CSC_BAD_ROW = 2,     // row < 0 or row >= n
    FW_CSC_UNSORTED = 4,    // row <= its predecessor in the column (unsorted or duplicate)
    FW_CSC_ZERO = 8,        // stored zero where counts are expected
    FW_CSC_NEGATIVE = 16,   // negative count
    FW_CSC_NONFINITE = 32   // NaN or +-Inf where real values are expected
};

__device__ inline int fw_wave_or(int v)
{
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// Flags of column j over the whole wavefront (every lane returns the same value); *a, *b = the column's entry range, empty when
// colptr is broken.
__device__ inline int fw_csc_check_column(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowval, int j, int n,
                                          long long nnz, int lane, long long *a, long long *b)
{
    const long long lo = colptr[j], hi = colptr[j + 1];
    if (lo < 0 || hi < lo || hi > nnz) {
        *a = *b = 0;
        return FW_CSC_BAD_COLPTR;
    }
    *a = lo;
    *b = hi;
    int bad = 0;
    for (long long e = lo + lane; e < hi; e += 64) {
        const int32_t r = rowval[e];
        if (r < 0 || r >= n) bad |= FW_CSC_BAD_ROW;
        if (e > lo && rowval[e - 1] >= r) bad |= FW_CSC_UNSORTED;
    }
    return fw_wave_or(bad);
}

inline const char *fw_csc_reason(int flags)
{
    if (flags & FW_CSC_BAD_COLPTR) return "colptr is not monotone within 0 .. nnz";
    if (flags & FW_CSC_BAD_ROW) return "a row index lies outside 0 .. n-1";
    if (flags & FW_CSC_UNSORTED) return "rows are not strictly ascending (unsorted or duplicate)";
    if (flags & FW_CSC_NONFINITE) return "non-finite value (NaN or Inf)";
    if (flags & FW_CSC_NEGATIVE) return "negative count";
    if (flags & FW_CSC_ZERO) return "stored zero";
    return "invalid";
}

#endif
