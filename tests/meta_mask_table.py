"""The table of the meta_mask tests (tests/test_meta_mask_cpu.py, tests/test_gpu_meta_mask.py): OTU counts with four meta variables
sitting between them, generated from a fixed seed.

200 samples x 48 OTU count columns, heterogeneous fill (a third of the cells zero: OTU pairs present nearly everywhere alternate with pairs absent from most samples), one sample
with exactly one non-zero OTU (its clr_nz value is 0.0f: a stored zero of the sparse front-end), and four meta columns at positions
3, 17, 30 and last of the full table:
  hab   0 / 1 habitat flag, shifts abundance and presence of OTUs 0..9
  cov   continuous, non-integral covariate tied to OTUs 10..13
  cat   integer category 0..3, tied to OTUs 14..16
  const the same number in every sample (must be dropped)
OTUs come in pairs that share a latent factor, so that OTU -- OTU edges exist in every mode.  The seed was fixed after checking, on the
CPU, that the oracle's network of the matrix the meta_data path normalises holds an edge with a meta endpoint and an edge between OTUs
in all four modes at max_k = 2 (test_meta_mask_cpu.py repeats that check)."""
import functools

import numpy as np

SEED = 2
N, P_OTU = 200, 48
CORE_BIAS, RARE_BIAS = 5.5, -1.0  # logit of presence at signal 0: about 3 % and 64 % zeros
META_NAMES = ["hab", "cov", "cat", "const"]


def meta_positions(p_otu):
    return [3, 17, 30, p_otu + 3]


@functools.lru_cache(maxsize=None)
def table(n=N, p_otu=P_OTU, seed=SEED):
    """-> (full table Float64 n x (p_otu + 4), mask, header, OTU block Int64, meta block Float64); never written to"""
    rng = np.random.default_rng(seed)
    hab = (rng.random(n) < 0.5).astype(np.float64)
    cov = rng.normal(0.0, 1.0, n) + 0.37
    cat = rng.integers(0, 4, n).astype(np.float64)
    const = np.full(n, 7.0)
    latent = rng.normal(0.0, 1.0, (n, (p_otu + 1) // 2))
    signal = 0.9 * latent[:, np.arange(p_otu) // 2] + 0.45 * rng.normal(0.0, 1.0, (n, p_otu))
    signal[:, 0:10] += 1.6 * (hab[:, None] - 0.5)
    signal[:, 10:14] += 1.1 * (cov[:, None] - 0.37)
    signal[:, 14:17] += 0.9 * (cat[:, None] - 1.5)
    counts = np.floor(np.exp(3.0 + 0.1 * rng.normal(0.0, 1.0, p_otu)[None, :] + signal)).astype(np.int64) + 1
    # absence follows the signal (presence / absence carries the structure for the discrete tests).  Heterogeneous fill: every other
    # pair of OTUs is nearly always present, the pairs between them are absent in most samples -- a third of the cells overall.  The
    # mi_nz test of two OTUs only sees the samples that hold both, and its automatic n_obs_min is 160 of the 200 samples
    # (hps * 4 * min(3^max_k, 8), learning.jl:51-57): a uniform fill of a third would leave no OTU pair testable.
    core = (np.arange(p_otu) // 2) % 2 == 0
    p_zero = 1.0 / (1.0 + np.exp(np.where(core, CORE_BIAS, RARE_BIAS)[None, :] + 1.6 * signal))
    counts[rng.random((n, p_otu)) < p_zero] = 0
    counts[0, :] = 0
    counts[0, 5] = 1  # the sample with one non-zero OTU (one read: log(1 / exp(log 1)) is 0.0 to the bit on any front-end)
    meta = np.stack([hab, cov, cat, const], axis=1)
    pos = meta_positions(p_otu)
    mask = np.zeros(p_otu + 4, dtype=bool)
    mask[pos] = True
    full = np.zeros((n, p_otu + 4), dtype=np.float64)
    full[:, ~mask], full[:, mask] = counts, meta
    header = np.empty(p_otu + 4, dtype=object)
    header[~mask], header[mask] = ["otu%d" % j for j in range(p_otu)], META_NAMES
    for a in (full, mask, counts, meta):
        a.setflags(write=False)
    return full, mask, [str(h) for h in header], counts, meta


def oracle_network(kind, mat, max_k=2):
    """the CPU oracle's network of a normalised matrix (single_il schedule) -> {(i, j): weight}"""
    from oracle import oracle as O
    if kind == "fz":
        o = O.Oracle("fz", cor_mat=O.cor(mat, "f32"), n_obs=mat.shape[0])
    elif kind == "fz_nz":
        o = O.Oracle("fz_nz", np.asarray(mat, dtype=np.float32))
    else:
        o = O.Oracle(kind, np.asarray(mat), sparse=True, max_k=max_k)
    try:
        return o.learn(max_k=max_k, feed_forward=True, round_size=1)["edges"]
    finally:
        o.close()


def edge_kinds(edges, meta_mask):
    """-> (edges with a meta endpoint, edges between OTUs)"""
    with_meta = sum(1 for i, j in edges if meta_mask[i] or meta_mask[j])
    return with_meta, len(edges) - with_meta
