"""Inputs shared by the k-means oracle pins (tests/test_oracle_cpu.py) and the op-level / whole-fit GPU tests
(tests/test_kmeans_ops_gpu.py): every one is regenerated from a seed, and every whole-fit input is one on which the
oracle's KMeans equals live sklearn (pinned on the CPU), so the GPU tests compare against the oracle alone."""
import numpy as np

from tests.golden import fixtures as FX

SQDIST_N = 400
SQDIST_CAND = [0, 5, 2, SQDIST_N - 1, 3]


def dup_rows(n, d, seed):
    """Rows ~ N(5, 3^2) (a mean far from 0: the three float64 sums cancel) with row 1 = row 0, row 2 = the next
    float32 after row 0 in every column, row 3 = row 0 * (1 + 1e-4): zero, one-ulp and small distances."""
    X = np.random.default_rng(seed).normal(5.0, 3.0, (n, d)).astype(np.float32)
    X[1] = X[0]
    X[2] = np.nextafter(X[0], np.float32(np.inf))
    X[3] = (X[0] * np.float32(1 + 1e-4)).astype(np.float32)
    return X


# Whole fits off the workload's shapes: (name, kind, n, d, true clusters, k, n_init).  trials = 2 + int(ln k);
# KMeans.fit runs restarts in groups of g = min(16, 64 // trials, LDS cap).
FIT_CASES = [
    ("blobs_n500_d37_k21_i13", "blobs", 500, 37, 9, 21, 13),      # trials 5 -> g 12: groups 12 + 1
    ("blobs_n300_d3_k5_i20", "blobs", 300, 3, 5, 5, 20),          # trials 3 -> g 16: groups 16 + 4
    ("blobs_n700_d130_k3_i17", "blobs", 700, 130, 3, 3, 17),      # groups 16 + 1, d % 4 = 2
    ("blobs_n260_d33_k4_i2", "blobs", 260, 33, 4, 4, 2),          # small-matrix E-step in the 4-row last chunk
    ("blobs_n333_d20_k55_i3", "blobs", 333, 20, 6, 55, 3),        # trials 6 -> g 10; d < 32
    ("overlap_n600_d37_k7_i13", "overlap", 600, 37, 7, 7, 13),
    ("overlap_n450_d5_k21_i13", "overlap", 450, 5, 6, 21, 13),    # groups 12 + 1
    ("overlap_n515_d33_k4_i3", "overlap", 515, 33, 4, 4, 3),      # last chunk of 3 rows: both remainders
    ("blobs_n200_d400_k3_i17", "blobs", 200, 400, 3, 3, 17),      # LDS cap: g = 15, groups 15 + 2
    ("repeat_n200_d19_k36_i3", "repeat", 200, 19, 3, 36, 3),      # 40 rows x 5, k = 36: empty clusters relocated
]
FIT_IDS = [c[0] for c in FIT_CASES]
RELOCATION_CASE = FIT_CASES[-1]


def fit_input(case):
    name, kind, n, d, true_k, k, n_init = case
    seed = n + d + k
    if kind == "blobs":
        return FX.blobs(n, d, true_k, seed)
    if kind == "overlap":
        return FX.overlap_blobs(n, d, true_k, 0.15, seed)
    # 40 rows x 5 copies, 8 of the rows a few float32 ulps from another one (x * (1 + 3e-6)).  With k = 36 nearly every
    # row seeds a centre; where both members of a near-duplicate pair do, the E-step's float32 rounding hands all their
    # copies to one of the two centres: the other cluster is empty while the largest row distance is > 0, and sklearn
    # relocates it to the farthest row.  (k-means++ never seeds two equal centres, so exact copies alone leave no
    # cluster empty.)  Seed and k were picked so that sklearn's own predict(X) equals its labels_ at the end.
    base = FX.blobs(n // 5, d, true_k, 5)
    for a in range(0, 16, 2):
        base[a + 1] = (base[a] * np.float32(1 + 3e-6)).astype(np.float32)
    return np.repeat(base, 5, axis=0)


def fit_groups(case):
    """The restart groups KMeans.fit runs for the case (cluster.KMeans.fit's lockstep group size)."""
    name, kind, n, d, true_k, k, n_init = case
    trials = 2 + int(np.log(k))
    g = max(1, min(16, 64 // trials, (150 * 1024) // (8 * trials * (d + 1))))
    return [min(g, n_init - g0) for g0 in range(0, n_init, g)]
