"""DBSCAN test helper: a numpy restatement of the rules the GPU DBSCAN is built to (sklearn 1.7.2, float32 input,
brute-force neighbourhoods), the seeded inputs of the fixture cases and the shape / exact-arithmetic cases.

Rules
  1. i and j are neighbours (self included) iff max(0, |x_i|^2 + |x_j|^2 - 2 x_i.x_j) <= r, every term float64 on the
     float32 rows upcast to float64, r = float64(float32(float32(eps) * float32(eps))) (the 32-bit distance metric
     squares the radius in float32).
  2. A point is core iff it has >= min_samples neighbours.
  3. Clusters are the connected components of the core-core neighbour graph, numbered in increasing order of their
     smallest core index; a non-core point with a core neighbour takes the smallest cluster number among its core
     neighbours; every other non-core point is -1.
A pair i < j is *borderline* when |d^2 - r| <= 4 (d + 4) 2^-53 (|x_i|^2 + |x_j|^2): only such a pair can be decided
differently by another summation order of the dot product.
"""
from __future__ import annotations

import numpy as np

LATENTS = "tests/golden/kmeans_latents_n1336_d128.npz"
MIN_SAMPLES = 5

# fixture inputs: name -> (n, d, seed); "latents" is the stored oracle latent matrix.  d = 8 is below sklearn's
# KD-tree switch (d <= 15), so its reference is DBSCAN(algorithm="brute").
BLOB_CASES = {
    "blobs_n1336_d64": (1336, 64, 11),
    "blobs_n2000_d128": (2000, 128, 12),
    "blobs_n777_d16": (777, 16, 13),
    "blobs_n1000_d32": (1000, 32, 14),
    "blobs_n900_d8": (900, 8, 15),
}
CASE_NAMES = ["latents"] + list(BLOB_CASES)


def fixture_path(name):
    return f"tests/golden/dbscan_{name}.npz"


def radius_sq(eps):
    e = np.float32(eps)
    return float(np.float32(e * e))


def density_blobs(n, d, seed):
    """Float32 blobs of uneven density: 4 Gaussian clusters whose points have individual scales (log-normal), so
    the k-distance curve is spread out and a radius leaves dense cores, a fringe of border points and noise."""
    rng = np.random.default_rng(seed)
    k = 4
    c = rng.normal(0.0, 4.0, (k, d))
    lab = rng.integers(0, k, n)
    scale = np.exp(rng.normal(0.0, 0.45, n))[:, None] * rng.uniform(0.7, 1.3, k)[lab][:, None]
    return (c[lab] + scale * rng.normal(0.0, 1.0, (n, d))).astype(np.float32)


def case_input(name):
    if name == "latents":
        return np.ascontiguousarray(np.load(LATENTS)["X"], dtype=np.float32)
    return density_blobs(*BLOB_CASES[name])


def sq_distances(X):
    """(d^2 [n][n] float64, |x|^2 [n] float64) by rule 1's expression."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    norms = np.einsum("ij,ij->i", X64, X64)
    sn = norms[:, None] + norms[None, :]
    return np.maximum(0.0, sn - 2.0 * (X64 @ X64.T)), norms


# quantiles of the k-distance curve the three radii of a case are read at (the latents are one diffuse cloud: only a
# small radius splits them into several dense cores)
QUANTILES = {"latents": (0.1, 0.5, 0.95)}
DEFAULT_QUANTILES = (0.5, 0.8, 0.95)


def k_distance_radii(X, quantiles=DEFAULT_QUANTILES, min_samples=MIN_SAMPLES):
    """Three radii from the k-distance curve (the distance to the min_samples-th neighbour, self included), rounded
    to 4 significant digits so that they are plain parameters."""
    d2, _ = sq_distances(X)
    kd = np.sqrt(np.sort(d2, axis=1)[:, min_samples - 1])
    return [float(f"{np.quantile(kd, q):.4g}") for q in quantiles]


def neighbourhoods(X, eps):
    """(adjacency bool [n][n], borderline pair count) for one radius."""
    d2, norms = sq_distances(X)
    r = radius_sq(eps)
    dim = np.asarray(X).shape[1]
    tol = (4.0 * (dim + 4) * 2.0 ** -53) * (norms[:, None] + norms[None, :])
    border = np.triu(np.abs(d2 - r) <= tol, k=1)
    return d2 <= r, int(border.sum())


def labels_from_adjacency(adj, min_samples):
    """(labels int64 [n], core indices ascending) by rules 2 and 3, from the neighbour bits alone."""
    n = adj.shape[0]
    core = adj.sum(axis=1) >= min_samples
    big = n
    cc = adj & core[:, None] & core[None, :]
    comp = np.where(core, np.arange(n), big)
    while True:   # every core point takes the smallest core index of its component
        new = np.where(cc, comp[None, :], big).min(axis=1, initial=big)
        new = np.minimum(comp, new)
        if np.array_equal(new, comp):
            break
        comp = new
    roots = np.flatnonzero(core & (comp == np.arange(n)))
    number = np.full(n + 1, -1, dtype=np.int64)
    number[roots] = np.arange(roots.size)
    labels = number[comp]
    # non-core points: the smallest cluster number among the core neighbours (numbers grow with the root index)
    near = np.where(adj & core[None, :], comp[None, :], big).min(axis=1, initial=big)
    labels = np.where(core, labels, number[near])
    return labels.astype(np.int64), np.flatnonzero(core)


def dbscan(X, eps, min_samples=MIN_SAMPLES):
    """(labels, core indices, borderline pair count) of the rules above."""
    adj, border = neighbourhoods(X, eps)
    labels, core = labels_from_adjacency(adj, min_samples)
    return labels, core, border


def stats(labels, core_idx):
    """(clusters, noise points, border points) of a labelling."""
    n_clusters = int(labels.max()) + 1 if labels.size else 0
    noise = int((labels == -1).sum())
    return n_clusters, noise, int(labels.size - noise - len(core_idx))


# ---------------------------------------------------------------------------------------------- exact cases
def lattice(side=6, d=16, seed=3):
    """side^3 integer lattice points (spacing 1) embedded in the first three of d coordinates, shuffled, plus an
    integer offset: every squared distance and every tested threshold is a small integer (exact in any order)."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    g = g[(g.sum(axis=1) % 5) != 0]          # holes: points of differing neighbour counts
    X = np.zeros((g.shape[0], d), dtype=np.float32)
    X[:, :3] = g
    X[:, 3:] = 2.0
    return X[rng.permutation(X.shape[0])]


def bridge(d=16):
    """Two integer crosses (a centre with 5 arms at distance 1: at eps = 1, min_samples = 5 the centre is core, the
    arms are border points) whose centres (1, 0, 0) and (3, 0, 0) are both at distance exactly 1 from one bridge
    point (2, 0, 0): a border point adjacent to the cores of two clusters.  Rows 0-5, 6-11 and 12."""
    arms = np.array([[0, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
    X = np.zeros((13, d), dtype=np.float32)
    X[:6, :3] = arms + np.array([1, 0, 0], dtype=np.float32)
    X[6:12, :3] = arms * np.array([-1, 1, 1], dtype=np.float32) + np.array([3, 0, 0], dtype=np.float32)
    X[12, :3] = [2, 0, 0]    # the bridge: 3 neighbours (itself and the two centres), not core
    return X
