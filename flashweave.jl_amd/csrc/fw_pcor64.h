// Float64 pcor_rec (statfuns.jl:23-75 with ContType = Float64, learn_network(prec = 64)): the arithmetic the Float64 kernels of
// fw_fz64.hip share with the host.  Every value is a Float64 from the first matrix entry on, so none of the mixed-type rules of the
// Float32 path (fw_fz_core.h) apply: one formula per level,
//     e = round5(a - b * c),  d = sqrt(1 - b * b) * sqrt(1 - c * c),  rho = d == 0 ? 0 : e / d,  clamped (< -1 -> -1, >= 1 -> 1),
// with a, b, c the three partial correlations one level below.  Only +, -, *, /, sqrt and rint are involved and each is correctly
// rounded on the host and on the device, so the value is the same bits wherever it is computed -- provided no a * b + c is
// contracted into a fused multiply-add (-ffp-contract=off in every unit that includes this file; the reference never fuses).
//
// __host__ __device__-clean like fw_unrank.h: tests/native/pcor64_check.cpp compiles it with g++ and compares it with the oracle.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define FW_P64_HD __host__ __device__ inline
#else
#define FW_P64_HD inline
#endif

#define FW_PCOR64_MAX_K 5  // sizes the Float64 path serves

// round(x, digits = 5) on a Float64: Base._round_digits -> round(x * 10^5) / 10^5, ties to even; x itself if that is not finite
FW_P64_HD double fw_round5_f64(double x)
{
    const double y = rint(x * 100000.0) / 100000.0;
    return (y - y == 0.0) ? y : x;  // (finite <=> y - y == 0; isfinite is a macro on some hosts and an overload set on the device)
}

FW_P64_HD double fw_clamp_pcor64(double v)  // statfuns.jl:58-62: a NaN stays
{
    if (v < -1.0) return -1.0;
    if (v >= 1.0) return 1.0;
    return v;
}

// one level of statfuns.jl:44-62: rho(A, B | S + z) from a = rho(A, B | S), b = rho(A, z | S), c = rho(B, z | S)
FW_P64_HD double fw_pcor64_step(double a, double b, double c)
{
    const double prod = b * c;
    const double e = fw_round5_f64(a - prod);
    const double bb = b * b;
    const double d1 = sqrt(1.0 - bb);
    const double cc = c * c;
    const double d2 = sqrt(1.0 - cc);
    const double denom = d1 * d2;
    return fw_clamp_pcor64(denom == 0.0 ? 0.0 : e / denom);
}

// rho(X, Y | z[0 .. k)), 1 <= k <= FW_PCOR64_MAX_K, on a p x p Float64 matrix.  The recursion of statfuns.jl:44-53 peels the LAST
// element first and asks for (X, Y | rest), (X, z_last | rest), (Y, z_last | rest): with U = [X, Y, z_k, ..., z_1] every pair it
// ever touches is (U[a], U[b]) with a < b, conditioned on a suffix of U.  Bottom-up: level j conditions every pair left of z_j on
// z_j, in place.  The matrix entry of a pair (A, B) is read where cor_mat[A, B] of a column-major matrix sits (cor[B * p + A]),
// so that a caller's matrix that is not exactly symmetric gives the reference's value too.
template <int K>
FW_P64_HD double fw_pcor64_k(const double *cor, long long p, int X, int Y, const int *z)
{
    constexpr int M = K + 2;  // (compile-time sizes: on the device the work matrix stays in registers)
    int U[M];
    double R[M][M];
    U[0] = X;
    U[1] = Y;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int q = 0; q < K; ++q) U[2 + q] = z[K - 1 - q];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int a = 0; a < M; ++a)
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int b = a + 1; b < M; ++b) R[a][b] = cor[(long long)U[b] * p + U[a]];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int last = M - 1; last >= 2; --last)  // condition on U[last] = z_1, z_2, ..., z_K
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (int a = 0; a < last; ++a)
#if defined(__HIPCC__)
#pragma unroll
#endif
            for (int b = a + 1; b < last; ++b) R[a][b] = fw_pcor64_step(R[a][b], R[a][last], R[b][last]);
    return R[0][1];
}

FW_P64_HD double fw_pcor64(const double *cor, long long p, int X, int Y, const int *z, int k)
{
    switch (k) {
        case 1: return fw_pcor64_k<1>(cor, p, X, Y, z);
        case 2: return fw_pcor64_k<2>(cor, p, X, Y, z);
        case 3: return fw_pcor64_k<3>(cor, p, X, Y, z);
        case 4: return fw_pcor64_k<4>(cor, p, X, Y, z);
        default: return fw_pcor64_k<5>(cor, p, X, Y, z);
    }
}
