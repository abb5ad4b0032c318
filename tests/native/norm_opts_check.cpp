// Host driver for the option validation of csrc/fw_norm_host.h (norm_opts_check): which fw_norm_opts a kind takes, and in which words
// it refuses the others (tests/test_norm_bins_cpu.py compiles and runs it, once plainly and once under -fsanitize=address,undefined).
// It reads one command per line from stdin, calls the header and prints what came back, one line per command; every check is the
// Python side's.
//   opts kind n_bins rank_method disc_method   -> ok b dense mean plain | refused <the words>
//   null kind                                  -> the same for a NULL fw_norm_opts (the defaults)
#include <cstdio>
#include <iostream>
#include <string>

#include "fw_norm_host.h"

static void answer(const char *no, const NormOpts &O)
{
    if (no)
        std::printf("refused %s\n", no);
    else
        std::printf("ok %d %d %d %d\n", O.b, (int)O.dense, (int)O.mean, (int)O.plain());
}

int main()
{
    std::string cmd;
    while (std::cin >> cmd) {
        int kind = 0;
        NormOpts O;
        O.b = -7;  // (norm_opts_check starts from the defaults whatever it is handed)
        if (cmd == "opts") {
            fw_norm_opts o{0, 0, 0};
            if (!(std::cin >> kind >> o.n_bins >> o.rank_method >> o.disc_method)) {
                std::fprintf(stderr, "FAIL: input ends inside a command\n");
                return 1;
            }
            answer(norm_opts_check(&o, norm_kind(kind), O), O);
        } else if (cmd == "null") {
            if (!(std::cin >> kind)) {
                std::fprintf(stderr, "FAIL: input ends inside a command\n");
                return 1;
            }
            answer(norm_opts_check(nullptr, norm_kind(kind), O), O);
        } else {
            std::fprintf(stderr, "FAIL: unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}
