// Host-side run of csrc/fw_pcor64.h (the Float64 pcor_rec the device kernels of fw_fz64.hip use), for tests/test_fz64_cpu.py.
// in : int32 p, int32 m, p * p doubles (column-major matrix), m records of 8 int32 {X, Y, k, z[0..4]}
// out: m doubles, the statistic of each test (k = 0: the matrix entry cor_mat[X, Y])
// Build with -ffp-contract=off, as the library is.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../flashweave.jl_amd/csrc/fw_pcor64.h"

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t hdr[2];
    if (fread(hdr, sizeof(int32_t), 2, f) != 2) return 2;
    const int p = hdr[0], m = hdr[1];
    std::vector<double> cor((size_t)p * p);
    if (fread(cor.data(), sizeof(double), cor.size(), f) != cor.size()) return 2;
    std::vector<int32_t> rec((size_t)m * 8);
    if (fread(rec.data(), sizeof(int32_t), rec.size(), f) != rec.size()) return 2;
    fclose(f);
    std::vector<double> out((size_t)m);
    for (int t = 0; t < m; ++t) {
        const int32_t *r = &rec[(size_t)t * 8];
        const int X = r[0], Y = r[1], k = r[2];
        int z[FW_PCOR64_MAX_K] = {r[3], r[4], r[5], r[6], r[7]};
        out[t] = k == 0 ? cor[(size_t)Y * p + X] : fw_pcor64(cor.data(), p, X, Y, z, k);
    }
    FILE *g = fopen(argv[2], "wb");
    if (!g) return 2;
    fwrite(out.data(), sizeof(double), out.size(), g);
    fclose(g);
    printf("ok %d\n", m);
    return 0;
}
