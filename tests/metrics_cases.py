"""Inputs shared by the metric-kernel GPU tests (tests/test_metrics_ops_gpu.py) and the CPU pins of their bounds
(tests/test_oracle_cpu.py): every one is regenerated from a seed.  Labels are always a permutation-patched
integers(0, k), so every label in [0, k) occurs: the kernels index with them unchecked."""
import numpy as np


def normals(n, d, seed, offset=0.0):
    X = np.random.default_rng(seed).normal(0.0, 1.0, (n, d)).astype(np.float32)
    return (X + np.float32(offset)).astype(np.float32)


def labels(n, k, seed):
    rng = np.random.default_rng(seed + 7919)
    y = rng.integers(0, k, n)
    y[rng.permutation(n)[:k]] = np.arange(k)
    return y.astype(np.int32)


# (id, n, d, k, offset)
SIL_CASES = (
    # DMAX dispatch edges 32|33, 64|65; d = 1; zero-padded float4 tails; the full 128
    [(f"d{d}", 203, d, 5, 0.0) for d in (1, 3, 31, 32, 33, 63, 64, 65, 127, 128)]
    # the 64-row block and the 64-row LDS tile: one row short, exact, one over; n = 3 = a pair and a singleton
    + [(f"n{n}", n, 12, 2, 0.0) for n in (3, 63, 64, 65, 127, 129, 257)]
    # label-window edges: 64 accumulator rows at DMAX 32 / 64, 62 at DMAX 128
    + [(f"d16_k{k}", 300, 16, k, 0.0) for k in (64, 65, 128, 129)]
    + [(f"d128_k{k}", 300, 128, k, 0.0) for k in (62, 63, 124, 125)]
    # k = n - 1: almost every S[i][c] is one float32 distance -- the per-pair bound, not an average
    + [(f"kmax_d{d}", 130, d, 129, 0.0) for d in (33, 128)]
    # far from the origin: a Gram form would lose the distances here, direct differences do not
    + [("offset1000_d65", 300, 65, 9, 1000.0), ("offset100_d33", 200, 33, 4, 100.0)]
)
SIL_IDS = [c[0] for c in SIL_CASES]


def sil_input(case):
    name, n, d, k, off = case
    X = normals(n, d, seed=1000 * n + 10 * d + k, offset=off)
    if n == 3:
        return X, np.array([0, 0, 1], dtype=np.int32), k
    return X, labels(n, k, seed=n + d + k), k


def sil_semantic_inputs():
    """name -> (X, labels as the caller passes them): sklearn's special cases."""
    rng = np.random.default_rng(5)
    X = rng.normal(0, 1, (203, 24)).astype(np.float32)
    y = rng.integers(0, 5, 203)
    out = {}
    ys = y.copy()
    ys[17] = 9
    out["singleton"] = (X, ys)                                     # s = 0 (nan_to_num)
    Xd = X.copy()
    Xd[y == 0] = Xd[np.flatnonzero(y == 0)[0]]
    out["duplicates"] = (Xd, y)                                    # a = 0, b > 0 -> s = 1
    y3 = y % 3
    Xi = X.copy()
    Xi[y3 < 2] = X[0]
    out["identical_rows_in_two_clusters"] = (Xi, y3)               # a = b = 0 -> s = 0
    out["dbscan_noise_label"] = (X, rng.integers(-1, 3, 203))
    out["string_labels"] = (X, np.array(["rock", "pop", "jazz"])[rng.integers(0, 3, 203)])
    return out


# (id, n, d, k, offset)
CLU_CASES = (
    # the column loop strides by the block's 256 threads: d = 257, 513 take a second and third trip
    [(f"d{d}", 400, d, 6, 0.0) for d in (1, 3, 64, 65, 257, 513)]
    # 64 blocks of ceil(n / 64) rows: most own none at n < 64; the last is short at 65, 130, 4097
    + [(f"n{n}_k{k}", n, 20, k, 0.0) for n, k in ((3, 2), (40, 5), (63, 2), (64, 5), (65, 2), (130, 5), (4097, 5))]
    # d = 4096: 3 labels per LDS window -> 1, 2 and 3 launches
    + [(f"d4096_k{k}", 40, 4096, k, 0.0) for k in (3, 4, 7)]
    + [("k1024", 1100, 2, 1024, 0.0),                              # exactly 64 KiB of LDS in clu_dist_kernel
       ("kmax_n90", 90, 20, 89, 0.0),
       ("offset1000", 400, 20, 6, 1000.0)]
)
CLU_IDS = [c[0] for c in CLU_CASES]


def clu_input(case):
    name, n, d, k, off = case
    X = normals(n, d, seed=77 * n + 3 * d + k, offset=off)
    if n == 3:
        return X, np.array([0, 1, 1], dtype=np.int32), k
    return X, labels(n, k, seed=n + d + k + 1), k


# (X, labels, Davies-Bouldin, Calinski-Harabasz) of sklearn 1.7: its branches for coincident centroids, zero
# intra-cluster distances and zero dispersion.  Every sum in them is exact in float64.
DEGENERATE = {
    "two_of_three_centroids_coincide": ([[-1], [1], [-2], [2], [5], [7]], [0, 0, 1, 1, 2, 2], 4.0 / 9.0, 6.0),
    "all_intra_distances_zero": ([[0], [0], [3], [3], [9], [9]], [0, 0, 1, 1, 2, 2], 0.0, 1.0),
    "all_centroids_coincide": ([[-1], [1], [-2], [2]], [0, 0, 1, 1], 0.0, 0.0),
}
