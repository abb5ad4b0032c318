"""The host job pool's plan, restated in Python (csrc/fw_pool_host.h: fw_pool_enum_size, fw_pool_first_window, fw_pool_seglen,
fw_pool_growth; csrc/fw_pool.cpp: fwi_pool_add, fwi_pool_launch) for the default Fisher-z constants and max_k = 3.
tests/test_pool_host_cpu.py holds the header to it; tests/test_gpu_fz_screen.py plans its batches with it."""
import math


def _job_ranks(a, max_tests=10_000_000):
    return min(math.comb(a, 3) + math.comb(a, 2) + a, max_tests)


def _plan(alens, max_tests=10_000_000):
    """Launches of a batch whose jobs all run to their last rank -> [(seglen, [(job, lo, hi)])]."""
    N = [_job_ranks(a, max_tests) for a in alens]
    nxt = [0] * len(alens)
    width = [16384 if a >= 64 else 256 for a in alens]
    out = []
    while True:
        live = [i for i in range(len(alens)) if nxt[i] < N[i]]
        if not live:
            return out
        wins = [(i, nxt[i], nxt[i] + min(width[i], N[i] - nxt[i])) for i in live]
        total = sum(h - l for _, l, h in wins)
        seglen = max(256, min(8192, -(-(total // 3072) // 256) * 256))
        out.append((seglen, wins))
        growth = 256 if total < (1 << 22) else (4 if len(live) > 2048 else 16)
        for i, _, h in wins:
            nxt[i] = h
            width[i] *= growth
