// Structure check of a CSC triple on the device, shared by the entry points that take one from the caller and read it in kernels
// (fw_normalize_*_csc and their _dev forms in fw_norm.hip, fw_set_data_csc_f32* and their _dev forms in fw_fz.hip; fw_set_data_csc_i32_dev
// in fw_mi.hip takes the column range from here and looks at rows and values in one loop of its own): one wavefront per column, one pass.
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

// *a, *b = the entry range of column j, empty when colptr is broken (-> false): 0 <= colptr[j] <= colptr[j+1] <= nnz.
__device__ inline bool fw_csc_column_range(const int64_t *__restrict__ colptr, int j, long long nnz, long long *a, long long *b)
{
    const long long lo = colptr[j], hi = colptr[j + 1];
    const bool good = lo >= 0 && lo <= hi && hi <= nnz;
    *a = good ? lo : 0;
    *b = good ? hi : 0;
    return good;
}

// Flags of column j over the whole wavefront (every lane returns the same value); *a, *b = the column's entry range, empty when
// colptr is broken.
__device__ inline int fw_csc_check_column(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rowval, int j, int n,
                                          long long nnz, int lane, long long *a, long long *b)
{
    if (!fw_csc_column_range(colptr, j, nnz, a, b)) return FW_CSC_BAD_COLPTR;
    const long long lo = *a, hi = *b;
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
