// Host check of csrc/fw_cscres.h, the position arithmetic of the CSC-resident fz_nz layout (tests/test_cscres_cpu.py compiles and
// runs it, once plainly and once under -fsanitize=address,undefined).  For random planes it builds base[p][W] and the row-sorted
// runs of values the way the layout is defined -- by walking every column row by row -- and asserts that the header's functions
// find every entry: fw_cscres_pos gives, for every set bit, the index of that entry in the run, fw_cscres_value its value, and
// 0.0f for every clear bit.  vals is a heap array of exactly max(nnz, 1) floats, so a position outside it is a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "fw_cscres.h"

static unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd()
{
    unsigned long long x = (rng_state += 0x9E3779B97F4A7C15ull);
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

#define REQUIRE(cond, ...)                         \
    do {                                           \
        if (!(cond)) {                             \
            std::fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);     \
            std::fprintf(stderr, "\n");            \
            std::exit(1);                          \
        }                                          \
    } while (0)

// one table: `p_random` columns of the given fill (per mille), then an empty column, a full column, a column whose only entry is
// row n-1, one whose only entry is row 0, and another empty column at the very end (its base equals nnz: nothing may be read there);
// specials = false leaves the five columns empty (with fill 0: a table without a single entry, vals is the one stand-in float)
static long long check_table(int n, int p_random, int fill_pm, bool specials = true)
{
    const int W = (n + 63) / 64, p = p_random + 5;
    std::vector<unsigned long long> plane((size_t)p * W, 0);
    auto set = [&](int c, int row) { plane[(size_t)c * W + (row >> 6)] |= 1ull << (row & 63); };
    for (int c = 0; c < p_random; ++c)
        for (int row = 0; row < n; ++row)
            if ((int)(rnd() % 1000) < fill_pm) set(c, row);
    if (specials) {
        for (int row = 0; row < n; ++row) set(p_random + 1, row);
        set(p_random + 2, n - 1);
        set(p_random + 3, 0);
    }
    // the definition: runs in column order, rows ascending; base = position of the first entry at or after row 64 w
    std::vector<float> run;
    std::vector<uint32_t> base((size_t)p * W, 0), where((size_t)p * n, 0xFFFFFFFFu);
    for (int c = 0; c < p; ++c)
        for (int row = 0; row < n; ++row) {
            if ((row & 63) == 0) base[(size_t)c * W + (row >> 6)] = (uint32_t)run.size();
            if ((plane[(size_t)c * W + (row >> 6)] >> (row & 63)) & 1ull) {
                where[(size_t)c * n + row] = (uint32_t)run.size();
                run.push_back((float)(1 + c * 131 + row));  // never 0.0f, distinct within a column
            }
        }
    const size_t nnz = run.size();
    std::unique_ptr<float[]> vals(new float[nnz ? nnz : 1]);  // exactly what the upload allocates
    vals[0] = 0.0f;
    for (size_t i = 0; i < nnz; ++i) vals[i] = run[i];
    long long checked = 0;
    for (int c = 0; c < p; ++c) {
        const unsigned long long *pc = plane.data() + (size_t)c * W;
        const uint32_t *bc = base.data() + (size_t)c * W;
        uint32_t popc_before = 0;
        for (int w = 0; w < W; ++w) {  // base is the column start plus the popcount of the words before w
            REQUIRE(bc[w] == bc[0] + popc_before, "n=%d column %d word %d: base %u, start %u + %u", n, c, w, bc[w], bc[0], popc_before);
            popc_before += (uint32_t)fw_cscres_popc(pc[w]);
        }
        for (int row = 0; row < n; ++row) {
            const bool on = (pc[row >> 6] >> (row & 63)) & 1ull;
            const float v = fw_cscres_value(pc, bc, vals.get(), row);
            if (on) {
                const uint32_t pos = fw_cscres_pos(pc[row >> 6], bc[row >> 6], row & 63);
                REQUIRE(pos == where[(size_t)c * n + row], "n=%d column %d row %d: position %u, run index %u", n, c, row, pos, where[(size_t)c * n + row]);
                REQUIRE(pos < nnz, "n=%d column %d row %d: position %u outside %zu", n, c, row, pos, nnz);
                REQUIRE(v == (float)(1 + c * 131 + row), "n=%d column %d row %d: value %g", n, c, row, (double)v);
            } else {
                REQUIRE(v == 0.0f, "n=%d column %d row %d: clear bit reads %g", n, c, row, (double)v);
            }
            ++checked;
        }
    }
    return checked;
}

int main()
{
    long long checked = 0;
    REQUIRE(fw_cscres_below(0) == 0ull && fw_cscres_below(63) == 0x7FFFFFFFFFFFFFFFull, "fw_cscres_below");
    const int sizes[] = {1, 63, 64, 65, 128, 130, 16448};
    for (int n : sizes)
        for (int fill_pm : {0, 30, 500, 1000}) checked += check_table(n, n > 1000 ? 3 : 7, fill_pm);
    checked += check_table(130, 4, 0, false);
    std::printf("ok %lld cells\n", checked);
    return 0;
}
