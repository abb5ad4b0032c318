"""The host job pool's plan, restated in Python (csrc/fw_pool_host.h: fw_pool_enum_size, fw_pool_first_window, fw_pool_seglen,
fw_pool_growth; csrc/fw_pool.cpp: fwi_pool_add, fwi_pool_launch) for the default Fisher-z constants; max_k defaults to 3.
tests/test_pool_host_cpu.py holds the header to it; tests/test_gpu_fz_screen.py plans its batches with it, tests/fzhk_edges_tables.py
the batches of the max_k 4-5 switch-point tests (jobs that stop: `stops`)."""
import math


def _job_ranks(a, max_tests=10_000_000, max_k=3):
    return min(sum(math.comb(a, s) for s in range(1, max_k + 1)), max_tests)


def _seglen(total, seg_target=0):
    return max(256, min(8192, -(-(total // (seg_target or 3072)) // 256) * 256))


def _plan(alens, max_tests=10_000_000, max_k=3, stops=None, seg_target=0):
    """Launches of a batch -> [(seglen, [(job, lo, hi)])].  stops[i]: the rank at which job i stops (it leaves the pool after the launch
    whose window holds that rank), None: the job runs to its last rank.  seg_target: FW_SEG_TARGET, 0 for the default."""
    N = [_job_ranks(a, max_tests, max_k) for a in alens]
    stops = stops if stops is not None else [None] * len(alens)
    nxt = [0] * len(alens)
    gone = [False] * len(alens)
    width = [16384 if a >= 64 else 256 for a in alens]
    out = []
    while True:
        live = [i for i in range(len(alens)) if nxt[i] < N[i] and not gone[i]]
        if not live:
            return out
        wins = [(i, nxt[i], nxt[i] + min(width[i], N[i] - nxt[i])) for i in live]
        total = sum(h - l for _, l, h in wins)
        out.append((_seglen(total, seg_target), wins))
        growth = 256 if total < (1 << 22) else (4 if len(live) > 2048 else 16)
        for i, _, h in wins:
            gone[i] = stops[i] is not None and stops[i] < h
            nxt[i] = h
            width[i] *= growth
