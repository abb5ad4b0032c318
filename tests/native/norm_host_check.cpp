// Host driver for csrc/fw_norm_host.h, the rules of the normalisation front-end that hold no device code
// (tests/test_norm_host_cpu.py compiles and runs it, once plainly and once under -fsanitize=address,undefined).  It reads commands
// from stdin -- numbers as C99 hex floats, so they arrive to the bit -- calls the header and prints what came back, one line per
// command; every check is the Python side's.
//   kinds                                         -> per kind 0..5 and 9: known i32 tss binned clr_mode emit_mode none_left
//   params kind n pk tie_rel tss, n x (S SL NZ RMIN [s32])
//                                                 -> refused reason sample | mask.., rows.., pseudo.., g..
//   reduce n, 64 n x rsum, rlog, rzero, rmin      -> S.., SL.., NZ.., RMIN..
//   keep pk p, pk x two, pk x cols                -> sel.., cols.., mask..  (the mask starts as all ones)
//   rownew n nk, nk x rows                        -> rownew..
//   ocolptr p pf, (p + 1) x colptr, pf x fcols    -> ocolptr..
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>

#include "fw_norm_host.h"

static double num()
{
    std::string t;
    if (!(std::cin >> t)) {
        std::fprintf(stderr, "FAIL: input ends inside a command\n");
        std::exit(1);
    }
    return std::strtod(t.c_str(), nullptr);
}
static int integer() { return (int)num(); }
template <typename T> static void line(const char *name, const std::vector<T> &v)
{
    std::printf("%s", name);
    for (const T &x : v) std::printf(" %a", (double)x);
    std::printf("\n");
}

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "kinds") {
            for (int kind : {0, 1, 2, 3, 4, 5, 9}) {
                const NormKind K = norm_kind(kind);
                std::printf("kind %d %d %d %d %d %d %d %s\n", kind, K.known, K.i32, K.tss, K.binned, K.clr_mode, K.emit_mode, K.none_left ? K.none_left : "-");
            }
        } else if (cmd == "params") {
            const int kind = integer(), n = integer(), pk = integer();
            const double tie_rel = num();
            const bool tss = integer() != 0;
            NormTotals T{std::vector<double>((size_t)n), std::vector<double>((size_t)n), std::vector<double>((size_t)n), std::vector<int64_t>((size_t)n)};
            std::vector<float> s32(tss ? (size_t)n : 0);
            for (int i = 0; i < n; ++i) {
                T.S[i] = num(), T.SL[i] = num(), T.NZ[i] = (int64_t)num(), T.RMIN[i] = num();
                if (tss) s32[i] = (float)num();
            }
            std::vector<uint8_t> mask((size_t)n, 7);
            NormRows R;
            const NormRefusal no = norm_row_params(kind, n, pk, tie_rel, T, tss ? &s32 : nullptr, mask.data(), R);
            if (no.reason) {
                std::printf("refused %d %s\n", no.sample, no.reason);
                continue;
            }
            line("mask", mask), line("rows", R.rows), line("pseudo", R.pseudo), line("g", R.g);
        } else if (cmd == "reduce") {
            const int n = integer();
            const size_t cn = (size_t)NORM_CHUNKS * n;
            std::vector<double> rsum(cn), rlog(cn), rmin(cn);
            std::vector<int32_t> rzero(cn);
            for (double &v : rsum) v = num();
            for (double &v : rlog) v = num();
            for (int32_t &v : rzero) v = integer();
            for (double &v : rmin) v = num();
            const NormTotals T = norm_reduce_chunks(n, rsum, rlog, rzero, rmin);
            line("S", T.S), line("SL", T.SL), line("NZ", T.NZ), line("RMIN", T.RMIN);
        } else if (cmd == "keep") {
            const int pk = integer(), p = integer();
            std::vector<int32_t> two((size_t)pk), cols((size_t)pk);
            for (int32_t &v : two) v = integer();
            for (int32_t &v : cols) v = integer();
            std::vector<uint8_t> mask((size_t)p, 1);
            line("sel", norm_keep_columns(two, cols, mask.data())), line("cols", cols), line("mask", mask);
        } else if (cmd == "rownew") {
            const int n = integer(), nk = integer();
            std::vector<int32_t> rows((size_t)nk);
            for (int32_t &v : rows) v = integer();
            line("rownew", norm_rownew(n, rows));
        } else if (cmd == "ocolptr") {
            const int p = integer(), pf = integer();
            std::vector<int64_t> colptr((size_t)p + 1);
            std::vector<int32_t> fcols((size_t)pf);
            for (int64_t &v : colptr) v = (int64_t)num();
            for (int32_t &v : fcols) v = integer();
            line("ocolptr", norm_out_colptr(colptr.data(), fcols));
        } else {
            std::fprintf(stderr, "FAIL: unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}
