"""t-SNE test helper: the seeded inputs, the exact references and the rounding bounds the GPU t-SNE is held to, and a
numpy restatement of each kernel (hlmc_tsne_* in include/hlmc.h).

Exact references
  kNN        squared distances by direct differences in longdouble, neighbours ordered by (distance, index).
  search     sklearn's _binary_search_perplexity restated in plain Python float64 (math.exp / math.log, the sums in
             sklearn's sequential order): it reproduces sklearn bit for bit (tests/test_tsne_cpu.py).
  joint P    scipy's P + P.T of the conditional matrix, divided by max(sum, eps), indices sorted.
  gradient   the dense float64 gradient, Z and KL of the objective at angle = 0,
             4 (a sum_j p_ij q_ij (y_i - y_j) - sum_j q_ij^2 (y_i - y_j) / Z), q_ij = 1 / (1 + |y_i - y_j|^2).
  update     a transcription of sklearn's _gradient_descent step on float32 arrays.

Bounds (u = 2^-53, v = 2^-24 the float32 unit roundoff), each counted from the kernel's arithmetic:
  distance   1.01 (d + 4) 2^-52 (|x_i|^2 + |x_j|^2): three float64 sums of d + 3 roundings at most in any order whose
             absolute terms add up to <= 2 (|x_i|^2 + |x_j|^2) (oracle/kmeans_oracle.py sqdist_bound without the float32
             rounding of its result).
  entropy    the margin of one search step (search_margin): with e = 2 u per exp / log / division (the device's float64
             exp and log are ASSUMED accurate to 2 ulp; the division is correctly rounded),
             |H' - H| <= 2 [(k + 3) + 2 |log s| + (2 k + 8) beta sd + 2 max_j(d_j beta) (1 + beta sd)] u.
             A row is borderline when some step's |H - log perplexity| - 1e-5 or H - log perplexity lies within it.
  cond. P    |p' - p| <= 4 (k + 8 + 2 max_j(d_j beta)) u p (exp of a rounded argument, one division, the k-term sum).
  P values   half a float32 spacing + 64 (k + n / 256 + 16) u of the value (two conditional values, one addition, the
             total's per-row and 256-way sums, one division).
  repulsion  a term q^2 dx carries (17 v) of its magnitude: dx one rounding, dx dx + dy dy 4 v, 1 + d2 one, rcp 1 ulp
             = 2 v (the ISA's documented accuracy of v_rcp_f32), q <= 7 v, q q 15 v, times dx 17 v; the float64
             accumulation adds n u.  REP_V = 18 v covers both; Z carries 8 v.
  gradient   4 [a (len + 8) u sum |p q dx| + REP_V sum q^2 |dx| / Z + 8 v |rep| / Z] + half a float32 spacing.
  KL         a 8 v (the relative error of Z under the logarithm, sum p = a) + (k + n / 256 + 64) u (|KL| + a).
  update     the float32 steps of the update applied to a gradient inside its bound (update_bounds).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
F32 = np.float32
U = 2.0 ** -53
V = 2.0 ** -24
EPS64 = float(np.finfo(np.float64).eps)
TINY32 = float(np.finfo(np.float32).tiny)
SEARCH_TOL = 1e-5
ZERO_SUM = float(np.float32(1e-8))      # sklearn's EPSILON_DBL is a C float
REP_V = 18.0 * V
Z_V = 8.0 * V

MAX_K = 512
ROW_BLOCK, COL_SLAB_MIN, COL_SLABS_MAX = 256, 256, 64


def n_neighbors(n, perplexity):
    return min(n - 1, int(3.0 * perplexity + 1))


def col_slab_len(n):
    per = -(-n // COL_SLABS_MAX)
    return max(COL_SLAB_MIN, -(-per // COL_SLAB_MIN) * COL_SLAB_MIN)


def align256(b):
    return -(-b // 256) * 256


def grad_workspace_offsets(n):
    """Byte offsets of the gradient part of the workspace (include/hlmc.h): part, rep, rowstat, grad, end."""
    slabs = -(-n // col_slab_len(n))
    part = 0
    rep = part + align256(slabs * 3 * n * 8)
    rowstat = rep + align256(3 * n * 8)
    grad = rowstat + align256(2 * n * 8)
    return dict(part=part, rep=rep, rowstat=rowstat, grad=grad, end=grad + align256(2 * n * 4), slabs=slabs)


# ------------------------------------------------------------------------------------------------ inputs
def blobs(n, d, centres, seed):
    """centres * 10 + N(0, 1), the labels cycling through the centres."""
    rng = np.random.default_rng(seed)
    C = rng.normal(0.0, 1.0, (centres, d)) * 10.0
    y = np.arange(n) % centres
    return (C[y] + rng.normal(0.0, 1.0, (n, d))).astype(F32), y


FIT_CASES = {
    "n300_d16": dict(n=300, d=16, centres=4, seed=101, perplexity=30.0),
    "n200_d7": dict(n=200, d=7, centres=3, seed=102, perplexity=10.0),
    "n1336_d64": dict(n=1336, d=64, centres=6, seed=103, perplexity=30.0),
}
FIT_FIXTURE = "tests/golden/tsne_fits.npz"


def fit_input(name):
    c = FIT_CASES[name]
    return blobs(c["n"], c["d"], c["centres"], c["seed"])


def gauss(n, d, seed, scale=1.0, offset=0.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(0.0, scale, (n, d)) + offset).astype(F32)


# name -> (n, d, k, kind); every n of {2, 63, 64, 65, 129, 300}, d of {1, 3, 33, 128} and k of {1, 16, 91, n - 1}
KNN_CASES = {
    "n2_d1_k1": (2, 1, 1, "gauss"),
    "n63_d3_k16": (63, 3, 16, "gauss"),
    "n64_d33_k63": (64, 33, 63, "gauss"),
    "n65_d128_k64": (65, 128, 64, "gauss"),
    "n129_d3_k91": (129, 3, 91, "gauss"),
    "n129_d33_k1": (129, 33, 1, "gauss"),
    "n300_d128_k91": (300, 128, 91, "gauss"),
    "n300_d33_k299": (300, 33, 299, "gauss"),
    "n300_d1_k16": (300, 1, 16, "gauss"),
    "offset_n129_d33_k16": (129, 33, 16, "offset"),
    "dups_n65_d3_k16": (65, 3, 16, "dups"),
}


def knn_input(name):
    n, d, k, kind = KNN_CASES[name]
    seed = 1000 + sum(map(ord, name))
    if kind == "offset":
        return gauss(n, d, seed, 1.0, 1000.0)
    X = gauss(n, d, seed)
    if kind == "dups":            # 20 copies of row 0, 10 of row 1: ties at distance 0 and among the copies
        X[2:22] = X[0]
        X[22:32] = X[1]
    return X


# ------------------------------------------------------------------------------------------------ kNN
def sqdist_exact(X):
    Xl = np.asarray(X, F32).astype(LD)
    D = np.zeros((X.shape[0], X.shape[0]), LD)
    for c in range(X.shape[1]):
        t = Xl[:, c][:, None] - Xl[:, c][None, :]
        D += t * t
    return D


def sqdist_bound(X):
    X64 = np.asarray(X, F32).astype(np.float64)
    nrm = (X64 * X64).sum(axis=1)
    return 1.01 * (X.shape[1] + 4) * 2.0 ** -52 * (nrm[:, None] + nrm[None, :])


def knn_from(D, k):
    """(indices [n][k], distances [n][k]) of the k smallest off-diagonal entries per row by (distance, index)."""
    D = np.array(D, copy=True)
    n = D.shape[0]
    D[np.arange(n), np.arange(n)] = np.inf
    idx = np.empty((n, k), np.int32)
    for i in range(n):
        idx[i] = np.lexsort((np.arange(n), D[i]))[:k]
    return idx, np.take_along_axis(D, idx.astype(np.int64), axis=1)


def knn_restated(X, k):
    """hlmc_tsne_knn in float64 numpy (the sums in numpy's order; the bound holds for any)."""
    X64 = np.asarray(X, F32).astype(np.float64)
    nrm = (X64 * X64).sum(axis=1)
    D = np.maximum(0.0, (nrm[:, None] + nrm[None, :]) - 2.0 * (X64 @ X64.T)) + 0.0
    return knn_from(D, k)


def knn_ambiguous_rows(D_exact, bound, k):
    """Rows whose exact k-th and (k+1)-th distances differ by no more than twice the bound (of either pair)."""
    n = D_exact.shape[0]
    if k >= n - 1:
        return np.zeros(n, bool)
    D = np.array(D_exact, np.float64)
    D[np.arange(n), np.arange(n)] = np.inf
    order = np.argsort(D, axis=1, kind="stable")
    a, b = order[:, k - 1], order[:, k]
    r = np.arange(n)
    return D[r, b] - D[r, a] <= 2.0 * np.maximum(bound[r, a], bound[r, b])


# ------------------------------------------------------------------------------------------------ perplexity search
def search_reference(d32, perplexity):
    """sklearn's _binary_search_perplexity on float32 squared distances [n][k], plain Python float64.
    Returns (P [n][k] float64, beta [n])."""
    d32 = np.asarray(d32, F32)
    n, k = d32.shape
    desired = math.log(float(F32(perplexity)))
    P = np.zeros((n, k))
    betas = np.zeros(n)
    for i in range(n):
        dist = [float(x) for x in d32[i]]
        beta_min, beta_max, beta = -math.inf, math.inf, 1.0
        p = [0.0] * k
        for _ in range(100):
            s = 0.0
            for j in range(k):
                p[j] = math.exp(-dist[j] * beta)
                s += p[j]
            if s == 0.0:
                s = ZERO_SUM
            sd = 0.0
            for j in range(k):
                p[j] /= s
                sd += dist[j] * p[j]
            diff = math.log(s) + beta * sd - desired
            if math.fabs(diff) <= SEARCH_TOL:
                break
            if diff > 0.0:
                beta_min = beta
                beta = beta * 2.0 if beta_max == math.inf else (beta + beta_max) / 2.0
            else:
                beta_max = beta
                beta = beta / 2.0 if beta_min == -math.inf else (beta + beta_min) / 2.0
        P[i] = p
        betas[i] = beta
    return P, betas


def wave_sum(a):
    """A wave's sum of a [rows][k] (k <= 512): lane l adds elements l, l + 64, ... in that order, then the xor
    butterfly 32, 16, .., 1."""
    rows, k = a.shape
    pad = np.zeros((rows, MAX_K))
    pad[:, :k] = a
    pad = pad.reshape(rows, MAX_K // 64, 64)
    v = pad[:, 0, :].copy()
    for u in range(1, MAX_K // 64):
        v = v + pad[:, u, :]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return v[:, 0]


def search_margin(k, s, beta, sd, dmax):
    return 2.0 * ((k + 3) + 2.0 * np.abs(np.log(s)) + (2 * k + 8) * beta * sd + 2.0 * dmax * beta * (1.0 + beta * sd)) * U


def search_restated(d32, perplexity):
    """hlmc_tsne_affinities' search in numpy, all rows at once in the wave's summation order.
    Returns (P, beta, borderline [n] bool, steps [n])."""
    d = np.asarray(d32, F32).astype(np.float64)
    n, k = d.shape
    desired = math.log(float(F32(perplexity)))
    beta = np.ones(n)
    bmin = np.full(n, -np.inf)
    bmax = np.full(n, np.inf)
    active = np.ones(n, bool)
    border = np.zeros(n, bool)
    steps = np.zeros(n, np.int64)
    P = np.zeros((n, k))
    dmax = d.max(axis=1)
    for _ in range(100):
        rows = np.flatnonzero(active)
        if rows.size == 0:
            break
        b = beta[rows]
        with np.errstate(under="ignore"):
            p = np.exp(-d[rows] * b[:, None])
        s = wave_sum(p)
        s[s == 0.0] = ZERO_SUM
        p = p / s[:, None]
        sd = wave_sum(d[rows] * p)
        diff = (np.log(s) + b * sd) - desired
        P[rows] = p
        steps[rows] += 1
        m = search_margin(k, s, b, sd, dmax[rows])
        border[rows] |= (np.abs(np.abs(diff) - SEARCH_TOL) <= m) | (np.abs(diff) <= m)
        done = np.abs(diff) <= SEARCH_TOL
        up = ~done & (diff > 0.0)
        down = ~done & ~up
        r = rows[up]
        bmin[r] = beta[r]
        beta[r] = np.where(np.isinf(bmax[r]), beta[r] * 2.0, (beta[r] + bmax[r]) / 2.0)
        r = rows[down]
        bmax[r] = beta[r]
        beta[r] = np.where(np.isinf(bmin[r]), beta[r] / 2.0, (beta[r] + bmin[r]) / 2.0)
        active[rows[done]] = False
    return P, beta, border, steps


def perplexity_of(d32, beta):
    """log-perplexity H of each row at the given beta, in longdouble."""
    d = np.asarray(d32, F32).astype(LD)
    b = np.asarray(beta, np.float64).astype(LD)[:, None]
    p = np.exp(-d * b)
    s = p.sum(axis=1)
    zero = s == 0
    s = np.where(zero, LD(ZERO_SUM), s)
    return (np.log(s) + b[:, 0] * (d * p).sum(axis=1) / s).astype(np.float64)


def cond_p_bound(P, d32, beta, k):
    dmax = np.asarray(d32, F32).astype(np.float64).max(axis=1) * beta
    return 4.0 * (k + 8 + 2.0 * dmax)[:, None] * U * P + 1e-300


def joint_reference(idx, cond):
    """sklearn's _joint_probabilities_nn from the neighbour lists and the conditional P: CSR (indptr int64, indices
    int32 sorted, float64 values), P + P.T over max(sum, eps)."""
    n, k = idx.shape
    rows = np.repeat(np.arange(n), k)
    P = sp.csr_matrix((np.asarray(cond, np.float64).ravel(), (rows, idx.ravel().astype(np.int64))), shape=(n, n))
    P = P + P.T
    P = sp.csr_matrix(P)
    P.sort_indices()
    P = P / np.maximum(P.sum(), EPS64)
    P = sp.csr_matrix(P)
    P.sort_indices()
    return P.indptr.astype(np.int64), P.indices.astype(np.int32), P.data.astype(np.float64)


def half_spacing32(v):
    a = np.abs(np.asarray(v, np.float64))
    f = a.astype(F32)
    f = np.where(f.astype(np.float64) > a, np.nextafter(f, F32(0)), f)
    return 0.5 * np.spacing(f).astype(np.float64)


def joint_value_bound(values64, n, k):
    return half_spacing32(values64) + 64.0 * (k + n / 256.0 + 16) * U * np.abs(values64)


def joint_restated(idx, cond):
    """The CSR build of hlmc_tsne_affinities in numpy: own entries and transposed-only entries, ranked by column,
    the total per row in column order and over the rows by block_sum_ordered; float32 values."""
    n, k = idx.shape
    rows = [dict() for _ in range(n)]
    member = [set(map(int, idx[i])) for i in range(n)]
    pos = [{int(c): t for t, c in enumerate(idx[i])} for i in range(n)]
    for j in range(n):
        for t in range(k):
            i = int(idx[j, t])
            if j in member[i]:
                v = cond[j, t] + cond[i, pos[i][j]]
            else:
                v = cond[j, t]
            if v == 0.0:                  # an underflowed exp: no entry, as scipy's P + P.T
                continue
            rows[j][i] = v
            if j not in member[i]:
                rows[i][j] = v
    indptr = np.zeros(n + 1, np.int64)
    indices, vals, rowsum = [], [], np.zeros(n)
    for i in range(n):
        cols = sorted(rows[i])
        indptr[i + 1] = indptr[i] + len(cols)
        s = 0.0
        for c in cols:
            s += rows[i][c]
            indices.append(c)
            vals.append(rows[i][c])
        rowsum[i] = s
    total = block_sum_ordered(rowsum)
    return indptr, np.asarray(indices, np.int32), (np.asarray(vals) / max(total, EPS64)).astype(F32)


def block_sum_ordered(x):
    """The device's one-block sum: thread t adds x[t], x[t + 256], ... in that order, then the tree 128, 64, .., 1."""
    x = np.asarray(x, np.float64)
    pad = np.zeros(-(-x.size // 256) * 256)
    pad[:x.size] = x
    sh = np.zeros(256)
    for row in pad.reshape(-1, 256):
        sh = sh + row
    st = 128
    while st > 0:
        sh[:st] = sh[:st] + sh[st:2 * st]
        st >>= 1
    return float(sh[0])


# ------------------------------------------------------------------------------------------------ gradient
def csr_dense(indptr, indices, values, n):
    return sp.csr_matrix((np.asarray(values, np.float64), indices, indptr), shape=(n, n)).toarray()


class GradRef:
    """Float64 reference of hlmc_tsne_gradient at Y (float32 [n][2]) for the CSR P and exaggeration a, with bounds."""

    def __init__(self, Y, indptr, indices, values, a=1.0):
        Y = np.asarray(Y, F32).astype(np.float64)
        n = Y.shape[0]
        P = csr_dense(indptr, indices, values, n) * a
        stored = csr_dense(indptr, indices, np.ones(len(values)), n) > 0
        diff = Y[:, None, :] - Y[None, :, :]
        q = 1.0 / (1.0 + (diff * diff).sum(axis=2))
        np.fill_diagonal(q, 0.0)
        self.Z = q.sum()
        z = max(self.Z, EPS64)
        q2 = q * q
        self.rep = (q2[:, :, None] * diff).sum(axis=1)
        self.attr = ((P * q)[:, :, None] * diff).sum(axis=1)
        self.grad = 4.0 * (self.attr - self.rep / z)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = P * np.log(np.maximum(P, TINY32) / np.maximum(q / z, TINY32))
        self.kl = float(t[stored].sum())
        self.kl_abs = float(np.abs(t[stored]).sum())
        self.gnorm = float(np.sqrt((self.grad.astype(F32).astype(np.float64) ** 2).sum()))
        rowlen = np.diff(indptr)[:, None]
        rep_abs = (q2[:, :, None] * np.abs(diff)).sum(axis=1)
        attr_abs = ((P * q)[:, :, None] * np.abs(diff)).sum(axis=1)
        self.rep_abs, self.attr_abs, self.z = rep_abs, attr_abs, z
        raw = 4.0 * ((rowlen + 8) * U * attr_abs + (REP_V + n * U) * rep_abs / z + Z_V * np.abs(self.rep) / z)
        self.grad_bound = raw + half_spacing32(np.abs(self.grad) + raw)
        self.Z_bound = (Z_V + n * U) * self.Z
        self.kl_bound = a * Z_V + (rowlen.max() + n / 256.0 + 64) * U * (abs(self.kl) + a)
        self.gnorm_bound = float(np.sqrt((self.grad_bound ** 2).sum())) + 64 * U * self.gnorm


def repulsion_restated(Y):
    """tsne_repulsion_kernel in numpy: float32 pair arithmetic operation by operation (the division correctly rounded
    where the kernel takes the 1-ulp reciprocal), float64 sums per slab.  Returns part [S][3][n]."""
    Y = np.asarray(Y, F32)
    n = Y.shape[0]
    L = col_slab_len(n)
    dx = Y[:, None, 0] - Y[None, :, 0]
    dy = Y[:, None, 1] - Y[None, :, 1]
    d2 = dx * dx + dy * dy
    q = F32(1.0) / (F32(1.0) + d2)
    np.fill_diagonal(q, F32(0.0))
    q2 = q * q
    tx, ty = (q2 * dx).astype(np.float64), (q2 * dy).astype(np.float64)
    parts = []
    for j0 in range(0, n, L):
        sl = slice(j0, min(n, j0 + L))
        parts.append(np.stack([tx[:, sl].sum(axis=1), ty[:, sl].sum(axis=1), q[:, sl].astype(np.float64).sum(axis=1)]))
    return np.stack(parts)


def combine_parts(part):
    """rep [3][n] = the slabs' partials added in slab order."""
    rep = np.zeros_like(part[0])
    for s in range(part.shape[0]):
        rep = rep + part[s]
    return rep


def gradient_restated(Y, indptr, indices, values, a=1.0):
    """hlmc_tsne_gradient in numpy: (grad float32 [n][2], Z, KL, |grad|)."""
    Y32 = np.asarray(Y, F32)
    n = Y32.shape[0]
    rep = combine_parts(repulsion_restated(Y32))
    Z = block_sum_ordered(rep[2])
    z = max(Z, EPS64)
    Y64 = Y32.astype(np.float64)
    grad = np.zeros((n, 2), F32)
    klrow, g2row = np.zeros(n), np.zeros(n)
    for i in range(n):
        sl = slice(indptr[i], indptr[i + 1])
        j = indices[sl]
        p = a * np.asarray(values[sl], np.float64)
        dx, dy = Y64[i, 0] - Y64[j, 0], Y64[i, 1] - Y64[j, 1]
        q = 1.0 / (1.0 + (dx * dx + dy * dy))
        ax, ay = (p * q * dx).sum(), (p * q * dy).sum()
        klrow[i] = (p * np.log(np.maximum(p, TINY32) / np.maximum(q / z, TINY32))).sum()
        grad[i] = F32(4.0 * (ax - rep[0, i] / z)), F32(4.0 * (ay - rep[1, i] / z))
        g2row[i] = float(grad[i, 0]) ** 2 + float(grad[i, 1]) ** 2
    return grad, Z, block_sum_ordered(klrow), math.sqrt(block_sum_ordered(g2row))


def exact_kl(indptr, indices, values, Y):
    """The exact float64 KL divergence of the embedding Y for the CSR P (sklearn's error term, all pairs in Z)."""
    return GradRef(np.asarray(Y, F32), indptr, indices, values, 1.0).kl


# ------------------------------------------------------------------------------------------------ update
def gradient_descent_step(p, update, gains, grad, momentum, learning_rate, min_gain=0.01):
    """sklearn's _gradient_descent loop body on float32 arrays, transcribed.  Returns new (p, update, gains)."""
    p, update, gains, grad = (np.array(a, F32, copy=True) for a in (p, update, gains, grad))
    inc = update * grad < 0.0
    dec = np.invert(inc)
    gains[inc] += 0.2
    gains[dec] *= 0.8
    np.clip(gains, min_gain, np.inf, out=gains)
    grad *= gains
    update = momentum * update - learning_rate * grad
    p += update
    return p, update, gains


def update_bounds(update, gains_new, grad, grad_bound, momentum, learning_rate):
    """|update' - update| and |p' - p| after one step when the gradient is within grad_bound and the gains agree:
    the product g * gains, the product with the learning rate, the product momentum * update and the difference each
    round once (4 v of the magnitudes), and the sum p + update once more."""
    g = np.abs(np.asarray(grad, np.float64)) + grad_bound
    mag = momentum * np.abs(np.asarray(update, np.float64)) + learning_rate * g * gains_new
    ub = learning_rate * gains_new * grad_bound * (1 + 4 * V) + 4 * V * mag
    return ub, ub + 2 * V * mag


# ------------------------------------------------------------------------------------------------ op-level cases
# name -> n, d, perplexity, data scale (wide: the first steps halve beta; narrow: they double it)
SEARCH_CASES = {"p5": (63, 3, 5.0, 1.0), "p30": (129, 7, 30.0, 1.0), "p100": (320, 5, 100.0, 1.0),
                "wide": (129, 7, 30.0, 300.0), "narrow": (129, 7, 30.0, 1e-3), "hub": (130, 32, 5.0, 1.0)}


def search_input(name):
    """(X, exact neighbour indices, float32 squared distances, perplexity) of a search case."""
    n, d, perp, scale = SEARCH_CASES[name]
    X = gauss(n, d, 77 + sum(map(ord, name)), scale)
    if name == "p5":
        X[1:40] = X[0]            # rows 0..39 coincide: every neighbour of such a row is at distance 0
    if name == "hub":             # row 0 at the centre of a shell: every other row lists it, its CSR row is full
        X[1:] = X[1:] / np.linalg.norm(X[1:], axis=1, keepdims=True) * (20.0 + X[1:, :1] * 0.3)
        X[0] = 0.0
    k = n_neighbors(n, perp)
    idx, d2 = knn_from(sqdist_exact(X).astype(np.float64), k)
    return X, idx, d2.astype(F32), perp


@functools.lru_cache(maxsize=None)
def csr_case(n, seed=5, perp=30.0, hub=False):
    """A CSR P of n rows from the restated kernels (hub: row 0 holds n - 1 entries)."""
    X = gauss(n, 32 if hub else 7, seed)
    if hub:
        X[1:] = X[1:] / np.linalg.norm(X[1:], axis=1, keepdims=True) * (20.0 + X[1:, :1] * 0.3)
        X[0] = 0.0
    k = n_neighbors(n, perp)
    idx, d2 = knn_from(sqdist_exact(X).astype(np.float64), k)
    cond, _, _, _ = search_restated(d2.astype(F32), perp)
    return joint_restated(idx, cond)


def grad_case(n, scale, seed=5, perp=30.0, hub=False):
    indptr, indices, values = csr_case(n, seed, perp, hub)
    Y = (np.random.default_rng(seed + 1).normal(0.0, 1.0, (n, 2)) * scale).astype(F32)
    return Y, indptr, indices, values


# ------------------------------------------------------------------------------------------------ sklearn's own P
def sklearn_joint(X, perplexity):
    """sklearn's joint probabilities for X (its kNN, its search, its symmetrisation): CSR with sorted indices."""
    from sklearn.manifold import _t_sne
    from sklearn.neighbors import NearestNeighbors
    n = X.shape[0]
    k = n_neighbors(n, perplexity)
    knn = NearestNeighbors(algorithm="auto", n_neighbors=k, metric="euclidean").fit(X)
    D = knn.kneighbors_graph(mode="distance")
    D.data **= 2
    P = sp.csr_matrix(_t_sne._joint_probabilities_nn(D, perplexity, 0))
    P.sort_indices()
    return P


@functools.lru_cache(maxsize=None)
def fit_fixture():
    return dict(np.load(FIT_FIXTURE))
