"""Ward test helper: a numpy restatement of the rules the GPU Ward clustering is built to (sklearn 1.7.2
``AgglomerativeClustering(n_clusters=k)`` = scipy 1.15 ``hierarchy.ward`` + sklearn's heap cut), the seeded inputs of
the fixture cases and the crafted distance matrices of the chain tests.

Rules
  1. Distances: float64 on the float32 rows upcast to float64.  Per pair s = 0, then for k = 0 .. d-1 in that order
     t = a_k - b_k, s = s + t * t (two roundings, no FMA), D = sqrt(s).
  2. Nearest-neighbour chain on the full symmetric matrix, n - 1 merges.  An empty chain starts at the lowest live
     index.  From the top x the scan starts at the chain predecessor (y, D[x][y]) (or (-1, +inf)), runs over the
     live i != x in increasing order and takes i only when D[x][i] is strictly smaller; the chain closes when y is
     the predecessor.  The pair is ordered x < y; (x, y, D[x][y], size[x] + size[y]) is recorded, x dies, y carries
     the merged cluster.
  3. Lance-Williams (Ward) for every live i != y, evaluated left to right without FMA:
       t = 1.0 / float64(ni + nx + ny)
       D[i][y] = sqrt(((ni + nx) * t) * dxi * dxi + ((ni + ny) * t) * dyi * dyi - (ni * t) * dxy * dxy)
  4. The merges are sorted by height with a stable sort; a union-find pass turns the representatives into cluster
     ids (row i creates cluster n + i), each children row is (min, max).
  5. Cut: a max-heap of node ids (heapq on negated ids) starting from the root, n_clusters - 1 rounds of push then
     pushpop; label i goes to the leaves under heap[i] in heap-array order.
"""
from __future__ import annotations

import heapq

import numpy as np

LATENTS = "tests/golden/kmeans_latents_n1336_d128.npz"
K_RANGE = range(2, 15)

# fixture inputs: name -> (kind, n, d, seed)
CASES = {
    "gauss_n300_d64": ("gauss", 300, 64, 21),
    "gauss_n257_d7": ("gauss", 257, 7, 22),
    "gauss_n64_d1": ("gauss", 64, 1, 23),
    "blobs_n200_d128": ("blobs", 200, 128, 24),
    "grid_n150_d3": ("grid", 150, 3, 25),
    "dups_n120_d16": ("dups", 120, 16, 26),
    "gauss_n2500_d16": ("gauss", 2500, 16, 27),
    "latents": ("latents", 1336, 128, 0),
}
CASE_NAMES = list(CASES)


def fixture_path(name):
    return f"tests/golden/ward_{name}.npz"


def case_input(name):
    kind, n, d, seed = CASES[name]
    rng = np.random.default_rng(seed)
    if kind == "latents":
        return np.ascontiguousarray(np.load(LATENTS)["X"], dtype=np.float32)
    if kind == "gauss":
        return rng.normal(0.0, 1.0, (n, d)).astype(np.float32)
    if kind == "blobs":      # four offset blobs far from the origin: large coordinates, small differences
        c = rng.normal(0.0, 6.0, (4, d)) + 1000.0
        return (c[rng.integers(0, 4, n)] + rng.normal(0.0, 1.0, (n, d))).astype(np.float32)
    if kind == "grid":       # integer coordinates: the matrix is full of exactly tied distances
        return rng.integers(0, 6, (n, d)).astype(np.float32)
    if kind == "dups":       # every row four times: zero distances, ties everywhere
        return np.repeat(rng.normal(0.0, 1.0, (n // 4, d)).astype(np.float32), 4, axis=0)
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------------ the rules
def pdist_full(X):
    """Rule 1: the full symmetric [n][n] float64 matrix."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    n, d = X64.shape
    s = np.zeros((n, n), np.float64)
    for k in range(d):
        t = X64[:, k][:, None] - X64[:, k][None, :]
        s = s + t * t
    return np.sqrt(s)


def ward_update(dxi, dyi, dxy, nx, ny, ni):
    """Rule 3 on arrays (ni int array; nx, ny ints)."""
    t = 1.0 / (ni + nx + ny).astype(np.float64)
    a = (((ni + nx).astype(np.float64) * t) * dxi) * dxi
    b = (((ni + ny).astype(np.float64) * t) * dyi) * dyi
    c = ((ni.astype(np.float64) * t) * dxy) * dxy
    with np.errstate(invalid="ignore"):
        return np.sqrt((a + b) - c)


def nn_chain(D):
    """Rules 2 and 3 on a full symmetric float64 matrix (copied).  Returns the raw merge records in merge order:
    (a int32 [n-1], b int32 [n-1], dist float64 [n-1], size int32 [n-1]).  Raises ValueError when a scan finds no
    neighbour (a NaN or +inf row)."""
    D = np.array(D, dtype=np.float64)
    n = D.shape[0]
    size = np.ones(n, np.int64)
    idx = np.arange(n)
    chain = []
    ma, mb = np.zeros(n - 1, np.int32), np.zeros(n - 1, np.int32)
    md, ms = np.zeros(n - 1, np.float64), np.zeros(n - 1, np.int32)
    for k in range(n - 1):
        if not chain:
            chain.append(int(np.flatnonzero(size > 0)[0]))
        while True:
            x = chain[-1]
            if len(chain) > 1:
                y = chain[-2]
                cur = D[x, y]
            else:
                y, cur = -1, np.inf
            live = (size > 0) & (idx != x)
            row = np.where(live, D[x], np.inf)
            with np.errstate(invalid="ignore"):
                row = np.where(row == row, row, np.inf)          # a NaN is smaller than nothing
            i = int(np.argmin(row))                                # first minimum = lowest index
            if row[i] < cur:
                y, cur = i, row[i]
            if y < 0:
                raise ValueError("nn_chain: a scan found no neighbour (NaN or infinite distances)")
            if len(chain) > 1 and y == chain[-2]:
                break
            if len(chain) >= n:
                raise ValueError("nn_chain: chain longer than n")
            chain.append(y)
        del chain[-2:]
        if x > y:
            x, y = y, x
        nx, ny = int(size[x]), int(size[y])
        ma[k], mb[k], md[k], ms[k] = x, y, cur, nx + ny
        size[x] = 0
        size[y] = nx + ny
        upd = (size > 0) & (idx != y)
        v = ward_update(D[x, upd], D[y, upd], cur, nx, ny, size[upd])
        D[y, upd] = v
        D[upd, y] = v
    return ma, mb, md, ms


def relabel(ma, mb, md, n):
    """Rule 4: (children int64 [n-1][2], distances float64 [n-1])."""
    order = np.argsort(md, kind="mergesort")
    parent = np.arange(2 * n - 1)

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    children = np.zeros((n - 1, 2), np.int64)
    for row, m in enumerate(order):
        a, b = find(int(ma[m])), find(int(mb[m]))
        children[row] = (min(a, b), max(a, b))
        parent[a] = parent[b] = n + row
    return children, md[order].copy()


def cut(children, n, n_clusters):
    """Rule 5: labels int64 [n]."""
    nodes = [-(int(max(children[-1])) + 1)]
    for _ in range(n_clusters - 1):
        a, b = children[-nodes[0] - n]
        heapq.heappush(nodes, -int(a))
        heapq.heappushpop(nodes, -int(b))
    labels = np.zeros(n, np.int64)
    for i, node in enumerate(nodes):
        stack, leaves = [-node], []
        while stack:
            v = stack.pop()
            if v < n:
                leaves.append(v)
            else:
                stack.extend(int(c) for c in children[v - n])
        labels[leaves] = i
    return labels


def ward(X):
    """(children, distances) of float32 rows X by rules 1 - 4."""
    ma, mb, md, _ = nn_chain(pdist_full(X))
    return relabel(ma, mb, md, X.shape[0])


# ------------------------------------------------------------------------------------------------ crafted matrices
def _symmetric(upper):
    D = np.triu(upper, 1)
    return D + D.T


def chain_matrices():
    """name -> full symmetric float64 matrix for the chain tests."""
    out = {}
    rng = np.random.default_rng(31)
    # small integers: most scans meet ties, many of them with the chain predecessor
    out["integer_ties"] = _symmetric(rng.integers(1, 4, (97, 97)).astype(np.float64))
    # all distances equal: every scan ties with the predecessor
    out["all_equal"] = _symmetric(np.full((33, 33), 2.0))
    # duplicate rows: blocks of zeros
    out["duplicate_zeros"] = pdist_full(np.repeat(rng.normal(0.0, 1.0, (20, 5)).astype(np.float32), 3, axis=0))
    out["n2"] = np.array([[0.0, 3.5], [3.5, 0.0]])
    # more than two elements per thread of a 1024-thread block
    out["n2500"] = pdist_full(rng.normal(0.0, 1.0, (2500, 4)).astype(np.float32))
    return out


def nan_matrix():
    """A matrix whose row 0 is all NaN: the first scan finds no neighbour."""
    D = _symmetric(np.random.default_rng(32).uniform(1.0, 2.0, (70, 70)))
    D[0, 1:] = np.nan
    D[1:, 0] = np.nan
    return D
