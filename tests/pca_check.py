"""PCA test helper: the seeded case inputs, the exact oracle and the rounding bounds the GPU PCA is held to, and a
float64 numpy restatement of the two kernels (hlmc_pca_cov, hlmc_pca_project in include/hlmc.h).

Exact oracle: the mean and the centred Gram matrix in longdouble, numpy.linalg.eigh of its float64 rounding, the
eigenvalues descending and clipped at 0, each component's entry of largest magnitude (first occurrence) positive
(sklearn's svd_flip(u_based_decision=False)).

Bounds (u = 2^-53; xc = x - mean, exact; the MFMA's 4-step inner sum is assumed to round each product and each
addition at most once, the assumption dbscan.hip's borderline bound rests on as well):
  mean     |m'_c - m_c| <= delta_c = n u mean_r |x_rc|   (n - 1 additions in any order and the division); the float32
           attribute adds half a float32 spacing.
  Gram     |G' - G|_ij <= (n + 8) u sum_r |xc_ri| |xc_rj| + n delta_i delta_j.  The kernel rounds once per centred
           factor, once per product and n - 1 times in the sums (n + 2 in all); a slightly wrong mean only adds the
           second-order term because sum_r xc_r = 0.
  project  half a float32 spacing of the exact value + (p + 6) u sum_c |a_c - off_c| |b_cj|  (the kernel: p + 2).
  eigen    |lam'_i - lam_i| <= E and ||v'_i - v_i||_2 <= 2 sqrt(2) E / gap_i (Davis-Kahan), gap_i from the exact
           eigenvalues, E = ||Gram bound||_F + 4 rho, rho = ||G V - V Lam||_F of numpy's eigh ON THE EXACT Gram matrix
           in longdouble (the host solver's own error; the factor 4 because the device matrix differs from the exact
           one in its low bits and LAPACK's backward error depends on the input at that level).
A component is compared only when its bound is <= 1e-7 (COMPONENT_BOUND_MAX): sklearn's float32 solvers sit near 1e-6,
so a bug cannot hide under the bound.
"""
from __future__ import annotations

import functools

import numpy as np

U = 2.0 ** -53
COMPONENT_BOUND_MAX = 1e-7
LD = np.longdouble

# name -> n, d, k (n_components as passed), kind, seed, spectrum ratio, whiten
CASES = {
    "ref_simple": dict(n=1336, d=370, k=32, kind="spectrum", seed=31, ratio=0.9),
    "ref_cvae": dict(n=1336, d=290, k=64, kind="spectrum", seed=32, ratio=0.95),
    "latents": dict(n=4096, d=128, k=16, kind="spectrum", seed=33, ratio=0.9),
    "offset": dict(n=300, d=37, k=5, kind="offset", seed=34, ratio=0.9),
    "wide": dict(n=50, d=70, k=10, kind="spectrum", seed=35, ratio=0.9),
    "wide_all": dict(n=50, d=70, k=None, kind="spectrum", seed=35, ratio=0.9),
    "d1": dict(n=65, d=1, k=1, kind="spectrum", seed=36, ratio=0.9),
    "n2": dict(n=2, d=3, k=1, kind="spectrum", seed=37, ratio=0.9),
    "full": dict(n=200, d=16, k=16, kind="spectrum", seed=38, ratio=0.9),
    "zero_col": dict(n=200, d=16, k=8, kind="zero_col", seed=39, ratio=0.9),
    "whiten": dict(n=200, d=16, k=8, kind="spectrum", seed=40, ratio=0.9, whiten=True),
    "frac": dict(n=300, d=37, k=0.9, kind="spectrum", seed=41, ratio=0.9),
}
CASE_NAMES = list(CASES)
FIXTURE_ROWS = 64          # rows of sklearn's transform kept in a fixture
CONSTANT = "constant"      # the all-constant input: pinned to sklearn by its own fixture, no bounds

SLAB_MIN, SLABS_MAX, TILE = 256, 128, 64


def fixture_path(name):
    return f"tests/golden/pca_{name}.npz"


def spectrum_data(n, d, seed, ratio, offset=0.0):
    """Gaussian rows with standard deviations 10 ratio^i along the columns of a seeded orthogonal matrix."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(0.0, 1.0, (d, d)))
    z = rng.normal(0.0, 1.0, (n, d)) * (10.0 * ratio ** np.arange(d))
    return (z @ q.T + offset).astype(np.float32)


def case_input(name):
    if name == CONSTANT:
        return np.full((20, 5), 2.5, np.float32)
    c = CASES[name]
    if c["kind"] == "offset":        # far from the origin: the centring must happen in float64
        return spectrum_data(c["n"], c["d"], c["seed"], c["ratio"], 1000.0)
    X = spectrum_data(c["n"], c["d"], c["seed"], c["ratio"])
    if c["kind"] == "zero_col":      # one column of zero variance (a nonzero constant)
        X[:, 5] = 3.0
    return X


def fresh_rows(name, rows=70):
    """Rows the model was not fitted on, from the case's distribution (another seed)."""
    c = CASES[name]
    X = spectrum_data(rows, c["d"], c["seed"] + 1000, c["ratio"], 1000.0 if c["kind"] == "offset" else 0.0)
    if c["kind"] == "zero_col":
        X[:, 5] = 3.0
    return X


def grid_input(n, d, seed=7):
    """Op-level edge grid: nonzero column means, so a row past n that leaked -mean would show."""
    rng = np.random.default_rng(seed + 1000 * n + d)
    return (rng.normal(0.0, 1.0, (n, d)) + rng.uniform(2.0, 9.0, d)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ slab geometry
def slab_len(n):
    per = -(-n // SLABS_MAX)
    return max(SLAB_MIN, -(-per // 32) * 32)


def tile_pairs(d):
    t = -(-d // TILE)
    return [(i, j) for i in range(t) for j in range(i, t)]


GRID_D = (15, 16, 17, 63, 64, 65, 129)
GRID_N = (31, 32, 33, SLAB_MIN - 1, SLAB_MIN, SLAB_MIN + 1, 2 * SLAB_MIN + 1)


# ------------------------------------------------------------------------------------------------ exact oracle
def exact_mean_gram(X):
    Xl = np.asarray(X, np.float32).astype(LD)
    mean = Xl.sum(axis=0) / LD(X.shape[0])
    xc = Xl - mean
    return mean, xc, xc.T @ xc


def mean_delta(X):
    X64 = np.asarray(X, np.float32).astype(np.float64)
    return X.shape[0] * U * np.abs(X64).mean(axis=0)


def gram_bound(X, xc=None):
    n = X.shape[0]
    if xc is None:
        xc = exact_mean_gram(X)[1]
    a = np.abs(np.asarray(xc, np.float64))
    dl = mean_delta(X)
    return (n + 8) * U * (a.T @ a) + n * np.outer(dl, dl)


def flip_rows(V):
    big = np.argmax(np.abs(V), axis=1)
    s = np.sign(V[np.arange(V.shape[0]), big])
    s[s == 0] = 1.0
    return V * s[:, None]


def eig_descending(G64):
    lam, vec = np.linalg.eigh(G64)
    order = np.argsort(-lam, kind="stable")
    return np.maximum(lam[order], 0.0), flip_rows(np.ascontiguousarray(vec[:, order].T)), lam[order], vec[:, order]


def resolve_k(k, ratio_all, m):
    if k is None:
        return m
    if isinstance(k, float):
        return min(m, int(np.searchsorted(np.cumsum(ratio_all), k, side="right")) + 1)
    return k


class Exact:
    """The exact PCA of X and every bound derived from it."""

    def __init__(self, X, k=None, whiten=False):
        X = np.asarray(X, np.float32)
        n, d = X.shape
        self.X, self.n, self.d, self.m, self.whiten = X, n, d, min(n, d), whiten
        self.mean_ld, self.xc_ld, self.G_ld = exact_mean_gram(X)
        self.mean = self.mean_ld.astype(np.float64)
        self.xc = self.xc_ld.astype(np.float64)
        self.G = self.G_ld.astype(np.float64)
        self.delta = mean_delta(X)
        self.gram_bound = gram_bound(X, self.xc_ld)
        lam, V, lam_raw, vec_raw = eig_descending(self.G)
        res = self.G_ld @ vec_raw.astype(LD) - vec_raw.astype(LD) * lam_raw.astype(LD)[None, :]
        self.rho = float(np.sqrt((res * res).sum()))
        self.E = float(np.linalg.norm(self.gram_bound)) + 4.0 * self.rho
        self.lam_all, self.V_all = lam, V
        gaps = np.full(d, np.inf)
        if d > 1:
            diff = lam[:-1] - lam[1:]
            gaps[:-1] = diff
            gaps[1:] = np.minimum(gaps[1:], diff)
        with np.errstate(divide="ignore"):
            self.comp_bound_all = np.where(gaps > 0, 2.0 * np.sqrt(2.0) * self.E / gaps, np.inf)
        var_all = lam[:self.m] / (n - 1)
        self.total = var_all.sum()
        self.ratio_all = var_all / self.total
        self.k = k = resolve_k(k, self.ratio_all, self.m)
        self.lam, self.V = lam[:k], V[:k]
        self.comp_bound = self.comp_bound_all[:k]
        self.comparable = self.comp_bound <= COMPONENT_BOUND_MAX
        self.variance = var_all[:k]
        self.ratio = self.ratio_all[:k]
        self.singular = np.sqrt(self.lam)
        self.noise = var_all[k:].mean() if k < self.m else 0.0
        # attribute bounds that follow from |lam' - lam| <= E
        e = self.E / (n - 1)
        self.variance_bound = np.full(k, e)
        self.ratio_bound = (e + self.ratio * self.m * e) / (self.total - self.m * e)
        self.singular_bound = np.minimum(np.sqrt(self.E), self.E / np.maximum(self.singular, 1e-300))
        self.noise_bound = e

    def scale(self):
        return np.maximum(np.sqrt(self.variance), float(np.finfo(np.float32).eps))

    def forward_matrix(self):
        B = self.V.T
        return B / self.scale()[None, :] if self.whiten else B

    def forward_matrix_bound(self):
        """Per-column 2-norm bound of the device's forward matrix against the exact one."""
        if not self.whiten:
            return self.comp_bound
        s = self.scale()
        ds = self.variance_bound / (2.0 * s) / (1.0 - self.variance_bound / s ** 2)   # |sqrt(v') - sqrt(v)|
        return self.comp_bound / s + ds / s ** 2 * 1.0000001

    def transform(self, rows):
        """Exact projection of float32 rows (longdouble) and its composed bound [r][k]."""
        rows = np.asarray(rows, np.float32)
        B = self.forward_matrix()
        want, pb = project_exact(rows, B, self.mean_ld, None)
        xc = rows.astype(np.float64) - self.mean
        norm = np.sqrt((xc * xc).sum(axis=1))
        bound = pb + norm[:, None] * self.forward_matrix_bound()[None, :] \
            + np.linalg.norm(self.delta) * np.sqrt((B * B).sum(axis=0))[None, :]
        return want, bound

    def inverse(self, T, t_bound):
        """Exact inverse_transform of the exact features T and its composed bound given the features' bound."""
        B = self.V * np.sqrt(self.variance)[:, None] if self.whiten else self.V
        want, pb = project_exact(np.asarray(T, np.float64), B, None, self.mean_ld, float_rows=False)
        cb = self.comp_bound if not self.whiten else \
            self.comp_bound * np.sqrt(self.variance) + self.variance_bound / (2 * np.sqrt(self.variance)) * 1.0000001
        bound = pb + t_bound @ np.abs(B) + (np.abs(np.asarray(T, np.float64)) * cb[None, :]).sum(axis=1)[:, None] \
            + self.delta[None, :]
        return want, bound


def half_spacing32(v):
    """Half the float32 spacing of the binade that holds |v|."""
    a = np.abs(np.asarray(v, np.float64))
    f = a.astype(np.float32)
    f = np.where(f.astype(np.float64) > a, np.nextafter(f, np.float32(0)), f)
    return 0.5 * np.spacing(f).astype(np.float64)


def project_exact(A, B, a_off, o_off, float_rows=True):
    """(A - a_off) B + o_off in longdouble (rounded to float64) and the projection bound."""
    A = np.asarray(A, np.float32) if float_rows else np.asarray(A)
    Al = A.astype(LD)
    if a_off is not None:
        Al = Al - np.asarray(a_off, LD)
    want = Al @ np.asarray(B, LD)
    if o_off is not None:
        want = want + np.asarray(o_off, LD)
    want = want.astype(np.float64)
    p = A.shape[1]
    mag = np.abs(Al.astype(np.float64)) @ np.abs(np.asarray(B, np.float64))
    return want, half_spacing32(want) + (p + 6) * U * mag


# ------------------------------------------------------------------------------------------------ kernel restatement
def cov_restated(X, rng=None):
    """hlmc_pca_cov in float64 numpy: the slab order of the header; inside a slab the rows are added in a random
    order when rng is given (the MFMA's order is its own; the bound holds for any)."""
    X = np.asarray(X, np.float32)
    n, d = X.shape
    L = slab_len(n)
    X64 = X.astype(np.float64)
    s = np.zeros(d)
    for r0 in range(0, n, L):
        blk = X64[r0:r0 + L]
        part = [np.add.reduce(blk[g::4], axis=0) if blk[g::4].size else np.zeros(d) for g in range(4)]
        s = s + (((part[0] + part[1]) + part[2]) + part[3])
    mean = s / n
    G = np.zeros((d, d))
    parts = []
    for r0 in range(0, n, L):
        xc = X64[r0:r0 + L] - mean
        if rng is not None:
            xc = xc[rng.permutation(xc.shape[0])]
        P = np.zeros((d, d))
        for r in range(xc.shape[0]):
            P = P + np.outer(xc[r], xc[r])
        parts.append(P)
        G = G + P
    return mean, G, parts


def project_restated(A, B, a_off, o_off):
    A64 = np.asarray(A, np.float32).astype(np.float64)
    if a_off is not None:
        A64 = A64 - a_off
    acc = np.zeros((A64.shape[0], B.shape[1]))
    for c in range(A64.shape[1]):
        acc = acc + A64[:, c][:, None] * B[c][None, :]
    if o_off is not None:
        acc = acc + o_off
    return acc.astype(np.float32)


@functools.lru_cache(maxsize=None)
def exact(name):
    c = CASES[name]
    return Exact(case_input(name), c["k"], c.get("whiten", False))
